// clean_host_check.cpp -- the host rules of mola_lidar_odometry_hip/MapCleaning.h and the key-frame round trip in a stand-alone program,
// meant to be built with -fsanitize=address,undefined (tools/clean_host_check.sh).  No device is asked for: the neighbour rule, the
// relative pose, the decision and removal on made-up votes, the options, the file round trip of a cleaned set, and clean_keyframes on a
// set without points.  Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/MapCleaning.h"

using namespace mola_hip;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> u(-20.0, 20.0);
  // ---- options
  MapCleaningOptions opt = MapCleaningOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText("map_cleaning:\n  max_views_per_frame: 3\n  max_view_distance: 12\n"));
  CHECK(opt.max_views_per_frame == 3 && opt.max_view_distance == 12.0 && opt.n_rings == 32);
  bool refused = false;
  try {
    (void)MapCleaningOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText("map_cleaning:\n  no_such_key: 1\n"));
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);
  // ---- neighbours: every list sorted, capped, within the distance, free of the frame itself and of frames without points
  for (int trial = 0; trial < 200; trial++) {
    const size_t K = 1 + rng() % 40;
    std::vector<double> poses(12 * K, 0.0);
    std::vector<uint8_t> has(K);
    for (size_t k = 0; k < K; k++) {
      poses[12 * k] = poses[12 * k + 5] = poses[12 * k + 10] = 1.0;
      poses[12 * k + 3] = u(rng); poses[12 * k + 7] = u(rng); poses[12 * k + 11] = 0.1 * u(rng);
      has[k] = rng() % 7 != 0;
    }
    const auto nb = cleaning_neighbours(poses, has, opt);
    CHECK(nb.size() == K);
    for (size_t i = 0; i < K; i++) {
      CHECK(nb[i].size() <= opt.max_views_per_frame && (has[i] || nb[i].empty()));
      for (size_t q = 0; q < nb[i].size(); q++) {
        const uint32_t j = nb[i][q];
        CHECK(j < K && j != i && has[j] && (q == 0 || nb[i][q - 1] < j));
        const double dx = poses[12 * j + 3] - poses[12 * i + 3], dy = poses[12 * j + 7] - poses[12 * i + 7], dz = poses[12 * j + 11] - poses[12 * i + 11];
        CHECK((dx * dx + dy * dy) + dz * dz <= 144.0);
      }
    }
  }
  CHECK(cleaning_neighbours({}, {}, opt).empty());
  // ---- relative pose: T_j^-1 T_i of two yawed poses, against the closed form
  {
    const double a = 0.3, b = -1.1;
    const double Ti[12] = {std::cos(a), -std::sin(a), 0, 4, std::sin(a), std::cos(a), 0, -2, 0, 0, 1, 0.5};
    const double Tj[12] = {std::cos(b), -std::sin(b), 0, -1, std::sin(b), std::cos(b), 0, 3, 0, 0, 1, 0.25};
    double T[12];
    cleaning_relative_pose(Ti, Tj, T);
    CHECK(std::fabs(T[0] - std::cos(a - b)) < 1e-12 && std::fabs(T[4] - std::sin(a - b)) < 1e-12 && std::fabs(T[11] - 0.25) < 1e-12);
    CHECK(std::fabs(T[3] - (std::cos(b) * 5 + std::sin(b) * -5)) < 1e-12);
  }
  // ---- decision and removal on made-up votes; the round trip of the result
  MapCleaningOptions def;
  CHECK(cleaning_removes(2u, def) && !cleaning_removes(1u, def) && !cleaning_removes(2u | 2u << 16, def) && cleaning_removes(3u | 2u << 16, def));
  CHECK(!cleaning_removes(0xFFFFFFFFu, def) && cleaning_removes(0xFFFFu, def));
  molahip_host::KeyFrameSet set;
  molahip_host::KeyFrameTarget t;
  t.name = "localmap"; t.class_name = "HashedVoxelPointCloud";
  t.params.voxel_size = 1.f; t.params.max_points_per_voxel = 20;
  set.maps.push_back(t);
  std::vector<uint32_t> votes;
  size_t expect_removed = 0;
  for (int k = 0; k < 5; k++) {
    molahip_host::KeyFrame f;
    f.timestamp = 10.0 + k;
    f.pose[3] = 2.0 * k;
    f.has_points = k != 2;
    if (f.has_points)
      for (int e = 0; e < (k == 3 ? 3 : 1); e++) {
        molahip_host::KeyFrameLayer l;
        const size_t n = k == 4 ? 0 : 100 + 37 * e;
        for (size_t p = 0; p < n; p++) { l.x.push_back((float)u(rng)); l.y.push_back((float)u(rng)); l.z.push_back((float)u(rng)); }
        f.layers.push_back(l);
      }
    set.frames.push_back(f);
  }
  molahip_host::KeyFrameSet cleaned = set;
  for (auto& f : cleaned.frames) {
    if (!f.has_points) continue;
    size_t n = 0;
    for (const auto& l : f.layers) n += l.x.size();
    votes.resize(n);
    size_t want = 0;
    for (auto& v : votes) {
      v = (rng() % 4) | (rng() % 3) << 16;
      want += cleaning_removes(v, def);
    }
    const size_t got = cleaning_apply(f, votes.data(), def);
    CHECK(got == want);
    expect_removed += got;
  }
  CHECK(expect_removed > 0);
  const std::string path = dir + "/clean_host_check.mhkf";
  molahip_host::write_keyframe_file(path, cleaned);
  const molahip_host::KeyFrameSet back = molahip_host::read_keyframe_file(path);
  CHECK(back.frames.size() == 5 && back.maps.size() == 1);
  for (size_t k = 0; k < 5; k++) {
    CHECK(back.frames[k].has_points == cleaned.frames[k].has_points && back.frames[k].layers.size() == cleaned.frames[k].layers.size());
    CHECK(back.frames[k].timestamp == set.frames[k].timestamp && back.frames[k].pose[3] == set.frames[k].pose[3]);
    for (size_t e = 0; e < back.frames[k].layers.size(); e++) CHECK(back.frames[k].layers[e].x == cleaned.frames[k].layers[e].x);
  }
  remove(path.c_str());
  // ---- a set without points: unchanged, no device asked for; an occupancy map: refused
  molahip_host::KeyFrameSet bare = set;
  for (auto& f : bare.frames) { f.has_points = false; f.layers.clear(); }
  const CleaningResult r = clean_keyframes(bare, def);
  CHECK(r.cleaned.frames.size() == 5 && r.report.points_in == 0 && r.report.toJson().find("\"points_removed\": 0") != std::string::npos);
  bare.maps[0].class_name = "CVoxelMap";
  refused = false;
  try {
    (void)clean_keyframes(bare, def);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);
  puts("ok");
  return 0;
}
