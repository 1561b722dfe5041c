// motion_host_check.cpp -- the host rules of mola_lidar_odometry_hip/GyroDeskew.h in a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tools/motion_host_check.sh).  No device is asked for: the gyro_deskew: options and their refusals,
// the buffer (drops, forgetting), build_motion_table over random streams, windows and segment counts (its coverage failures
// included) with the properties the rule promises, and the --gyro-file parser.  Exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <string>

#include "mola_lidar_odometry_hip/GyroDeskew.h"

using namespace mola_hip;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

template <class F>
static bool refuses(F&& f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

int main() {
  std::mt19937 rng(13);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  // ---- options
  auto from = [](const std::string& text) { return GyroDeskewOptions::FromConfig(mp2p_icp_hip::Config::FromYamlText(text)); };
  const GyroDeskewOptions d = from("");
  CHECK(!d.enabled && d.window[0] == -0.06 && d.window[1] == 0.06 && d.segments == 12 && d.max_gap == 0.02 && d.time_zero_offset == 0.0);
  CHECK(d.gyro_bias[0] == 0.0 && d.sensor_rotation[0] == 1.0 && d.sensor_rotation[4] == 1.0 && d.sensor_rotation[8] == 1.0 && d.buffer_seconds == 2.0);
  const GyroDeskewOptions o = from("gyro_deskew:\n  enabled: true\n  window: [-0.1, 0.02]\n  segments: 64\n  max_gap: 0.004\n  time_zero_offset: -0.05\n"
                                   "  gyro_bias: [0.01, -0.02, 0.03]\n  sensor_rotation: [0, -1, 0, 1, 0, 0, 0, 0, 1]\n  buffer_seconds: 0.5\n");
  CHECK(o.enabled && o.window[0] == -0.1 && o.window[1] == 0.02 && o.segments == 64 && o.max_gap == 0.004 && o.time_zero_offset == -0.05);
  CHECK(o.gyro_bias[2] == 0.03 && o.sensor_rotation[1] == -1.0 && o.sensor_rotation[3] == 1.0 && o.buffer_seconds == 0.5);
  for (const char* bad : {"no_such_key: 1", "enabled: maybe", "window: [0.06, -0.06]", "window: [0]", "window: 1", "window: [nan, 1]", "segments: 0",
                          "segments: 65", "segments: 1.5", "segments: x", "max_gap: 0", "time_zero_offset: inf", "gyro_bias: [0, 0]",
                          "sensor_rotation: [2, 0, 0, 0, 1, 0, 0, 0, 1]", "sensor_rotation: [1, 0, 0, 0, 1, 0, 0, 0, -1]", "buffer_seconds: 0"})
    CHECK(refuses([&] { (void)from(std::string("gyro_deskew:\n  ") + bad + "\n"); }));
  CHECK(refuses([&] { (void)from("gyro_deskew: 3\n"); }));

  // ---- the buffer
  {
    GyroBuffer b(0.5);
    const double w[3] = {0.1, 0.2, 0.3}, bad[3] = {0.0, NAN, 0.0};
    CHECK(b.push(1.0, w) && !b.push(1.0, w) && !b.push(0.5, w) && !b.push(NAN, w) && !b.push(1.1, bad) && b.push(1.1, w));
    CHECK(b.size() == 2 && b.dropped() == 4);
    for (int k = 0; k < 1000; k++) b.push(1.2 + 0.0025 * k, w);
    CHECK(b.size() == 201 && b.samples().back().t - b.samples().front().t <= 0.5 + 1e-9);
    b.clear();
    CHECK(b.size() == 0 && b.dropped() == 0);
    const double v[3] = {0, 0, 0};
    CHECK(!build_motion_table(b, 1.0, d, v));  // an empty buffer covers nothing
  }

  // ---- the builder
  size_t tables = 0, none = 0;
  for (int it = 0; it < 400; it++) {
    GyroDeskewOptions q = d;
    q.segments = 1 + (uint32_t)(rng() % 64);
    q.window[0] = -0.15 + 0.2 * U(rng);
    q.window[1] = q.window[0] + 0.01 + 0.14 * U(rng);
    q.max_gap = (it % 3 == 0) ? 0.004 : 0.02;
    q.time_zero_offset = 0.04 * U(rng) - 0.02;
    q.buffer_seconds = (it % 5 == 0) ? 0.3 : 2.0;
    for (double& c : q.gyro_bias) c = 0.1 * U(rng) - 0.05;
    q.validate();
    const double stamp = 2.0e5 * U(rng), hz = (it % 4 == 0) ? 50.0 : ((it % 4 == 1) ? 1000.0 : 400.0);
    GyroBuffer b(q.buffer_seconds);
    const double start = stamp - 0.1 - 0.2 * U(rng), end = stamp + 0.4 * U(rng);
    const double hole = start + U(rng) * 0.6;
    for (double t = start; t < end; t += (1.0 + 0.2 * (U(rng) - 0.5)) / hz) {
      if (it % 3 == 1 && t > hole && t < hole + 0.03) continue;
      const double w[3] = {3.0 * std::sin(40.0 * t), 2.0 * std::cos(25.0 * t + 1.0), 1.5 * std::sin(11.0 * t + 2.0)};
      b.push(t, w);
    }
    const double v[3] = {U(rng), -U(rng), 0.5};
    const auto tab = build_motion_table(b, stamp, q, v);
    if (!tab) {
      none++;
      continue;
    }
    tables++;
    CHECK(tab->segments.size() == q.segments && tab->v[0] == v[0] && tab->v[1] == v[1] && tab->v[2] == v[2]);
    const mh_motion_table view = tab->table();
    CHECK(view.n_segments == q.segments && view.segments == tab->segments.data() && view.reserved_ == 0);
    CHECK(tab->segments[0].knot == q.window[0]);
    for (size_t s = 0; s < tab->segments.size(); s++) {
      const mh_motion_segment& g = tab->segments[s];
      CHECK(s == 0 || g.knot > tab->segments[s - 1].knot);
      CHECK(g.knot < q.window[1]);
      for (int a = 0; a < 3; a++) CHECK(std::isfinite(g.w[a]) && std::fabs(g.w[a]) < 7.0);  // a mean of rates bounded by 3 + 2 + 1.5 (+ bias)
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          double dot = 0;
          for (int k = 0; k < 3; k++) dot += g.R[i * 3 + k] * g.R[j * 3 + k];
          CHECK(std::fabs(dot - (i == j ? 1.0 : 0.0)) < 1e-12);
        }
    }
  }
  CHECK(tables > 100 && none > 30);

  // ---- the text form
  {
    const auto g = parse_gyro_text("# t wx wy wz\n10.0 0.1 0.2 0.3\n\n  10.0025\t-1e-3 0 2.5   # trailing\n#c\n10.005 0 0 0");
    CHECK(g.size() == 3 && g[0].t == 10.0 && g[1].w[0] == -1e-3 && g[1].w[2] == 2.5 && g[2].t == 10.005);
    CHECK(parse_gyro_text("").empty() && parse_gyro_text("\n\n# nothing\n").empty());
    for (const char* bad : {"1 0 0\n", "1 0 0 0 0\n", "1 0 x 0\n", "1 0 0 nan\n", "1 0 0 1e999\n"}) CHECK(refuses([&] { (void)parse_gyro_text(bad); }));
    CHECK(refuses([] { (void)read_gyro_file("/no/such/dir/gyro.txt"); }));
  }
  printf("ok: %zu tables, %zu scans without coverage\n", tables, none);
  return 0;
}
