// live_host_check.cpp -- the host rules of mola_lidar_odometry_hip/LiveMapCleaning.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/live_host_check.sh).  No device is asked for: the online_map_cleaning: options with their
// refusals, and the ring and neighbour rule (LiveRing) against a plain restatement on random pose lists, the wrap at max_views
// included.  Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/LiveMapCleaning.h"

using namespace mola_hip;
using mp2p_icp_hip::Config;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static bool refused(const std::string& text) {
  try {
    (void)OnlineMapCleaningOptions::FromConfig(Config::FromYamlText(text));
  } catch (const std::runtime_error& e) {
    return std::string(e.what()).rfind("online_map_cleaning: ", 0) == 0;
  }
  return false;
}

int main() {
  // ---- options
  const OnlineMapCleaningOptions def = OnlineMapCleaningOptions::FromConfig(Config::FromYamlText("other: 1\n"));
  CHECK(!def.enabled && def.max_views == 24 && def.every_n_updates == 1 && def.view_layer.empty() && def.target_maps.empty() && def.n_rings == 32);
  const OnlineMapCleaningOptions o = OnlineMapCleaningOptions::FromConfig(Config::FromYamlText(
      "online_map_cleaning:\n  enabled: true\n  max_views: 5\n  every_n_updates: 2\n  max_view_distance: 7.5\n  view_layer: decimated_for_icp\n"
      "  target_maps: [a, b]\n  win_rings: 1\n"));
  CHECK(o.enabled && o.max_views == 5 && o.every_n_updates == 2 && o.max_view_distance == 7.5 && o.view_layer == "decimated_for_icp");
  CHECK(o.target_maps.size() == 2 && o.target_maps[1] == "b" && o.win_rings == 1 && o.deviceParams().n_sectors == 128);
  for (const char* bad : {"no_such_key: 1", "max_views: 0", "max_views: 65", "every_n_updates: 0", "enabled: perhaps", "n_rings: 0", "max_views_per_frame: 3",
                          "target_maps: a", "target_maps: [a, a]", "min_through_votes: 0", "agree_weight: 1.5", "win_sectors: 3"})
    CHECK(refused(std::string("online_map_cleaning:\n  ") + bad + "\n"));
  // ---- the ring and the neighbour rule
  std::mt19937 rng(11);
  std::uniform_real_distribution<double> step(-4.0, 4.0);
  for (int trial = 0; trial < 300; trial++) {
    const uint32_t max_views = 1 + rng() % 9, every = 1 + rng() % 4;
    const double dist = (double)(rng() % 4) * 5.0;
    LiveRing ring(max_views, every);
    std::vector<std::vector<double>> kept(max_views);  // the restatement: the pose each slot holds
    double p[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const size_t K = 1 + rng() % 50;
    for (size_t u = 0; u < K; u++) {
      p[3] += step(rng); p[7] += step(rng); p[11] += 0.1 * step(rng);
      const LiveRing::Step st = ring.put(p);
      CHECK(st.slot == u % max_views && st.due == ((u + 1) % every == 0));
      kept[st.slot].assign(p, p + 12);
      CHECK(ring.updates() == u + 1 && ring.kept() == std::min<size_t>(u + 1, max_views));
      std::vector<uint32_t> want;
      for (uint32_t s = 0; s < max_views; s++) {
        if (kept[s].empty()) continue;
        const double dx = kept[s][3] - p[3], dy = kept[s][7] - p[7], dz = kept[s][11] - p[11];
        if ((dx * dx + dy * dy) + dz * dz <= dist * dist) want.push_back(s);
      }
      CHECK(ring.neighbours(p, dist) == want);
      CHECK(!want.empty() && std::find(want.begin(), want.end(), st.slot) != want.end());  // the update's own slot is always in
      for (uint32_t s : want)
        for (int e = 0; e < 12; e++) CHECK(ring.pose(s)[e] == kept[s][e]);
    }
    ring.clear();
    CHECK(ring.updates() == 0 && ring.kept() == 0 && ring.neighbours(p, 1e9).empty());
  }
  printf("ok\n");
  return 0;
}
