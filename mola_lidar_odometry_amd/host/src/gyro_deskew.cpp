// gyro_deskew.cpp -- see mola_lidar_odometry_hip/GyroDeskew.h.  Host logic only: no device call here.
#include "mola_lidar_odometry_hip/GyroDeskew.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <sstream>
#include <stdexcept>

#include "config_block.h"
#include "map_files.h"

namespace mola_hip {

using mp2p_icp_hip::Config;
using mp2p_icp_hip::CPose3D;

namespace {

const char* const kBlock = "gyro_deskew";

[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }

// 3x3 row-major
void mul33(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

void exp_so3(const double w[3], double scale, double* R) {
  const double u[3] = {w[0] * scale, w[1] * scale, w[2] * scale}, zero[3] = {0, 0, 0};
  const CPose3D p = CPose3D::FromRotVecAndTranslation(u, zero);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = p.T[i * 4 + j];
}

}  // namespace

// ================================================================== options
GyroDeskewOptions GyroDeskewOptions::FromConfig(const Config& cfg) {
  GyroDeskewOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    if (cfg[kBlock].kind != Config::Kind::Map) throw std::runtime_error(std::string(kBlock) + ": the block must be a map of keys");
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"enabled", "window", "segments", "max_gap", "time_zero_offset", "gyro_bias", "sensor_rotation", "buffer_seconds"});
    c.boolean("enabled", o.enabled);
    c.numbers("window", o.window, 2);
    double K = o.segments;
    c.number("segments", K);
    if (!(K >= 1.0) || !(K <= (double)MH_MOTION_MAX_SEGMENTS) || K != std::floor(K)) bad("segments", "must be an integer in 1 .. 64");
    o.segments = (uint32_t)K;
    c.number("max_gap", o.max_gap);
    c.number("time_zero_offset", o.time_zero_offset);
    c.numbers("gyro_bias", o.gyro_bias, 3);
    c.numbers("sensor_rotation", o.sensor_rotation, 9);
    c.number("buffer_seconds", o.buffer_seconds);
  }
  o.validate();
  return o;
}

void GyroDeskewOptions::validate() const {
  if (!std::isfinite(window[0]) || !std::isfinite(window[1]) || !(window[0] < window[1])) bad("window", "must be [lo, hi] with finite lo < hi");
  if (!(window[1] - window[0] <= 10.0)) bad("window", "must not span more than 10 s");
  if (segments < 1 || segments > MH_MOTION_MAX_SEGMENTS) bad("segments", "must be an integer in 1 .. 64");
  if (!(max_gap > 0.0) || !std::isfinite(max_gap)) bad("max_gap", "must be finite and > 0");
  if (!std::isfinite(time_zero_offset)) bad("time_zero_offset", "must be finite");
  for (double b : gyro_bias)
    if (!std::isfinite(b)) bad("gyro_bias", "must be finite");
  for (double r : sensor_rotation)
    if (!std::isfinite(r)) bad("sensor_rotation", "must be finite");
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double d = 0;
      for (int k = 0; k < 3; k++) d += sensor_rotation[i * 3 + k] * sensor_rotation[j * 3 + k];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-6)) bad("sensor_rotation", "must be a rotation matrix (row-major, orthonormal to 1e-6)");
    }
  const double* R = sensor_rotation;
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0.0)) bad("sensor_rotation", "must be a rotation matrix (determinant +1)");
  if (!(buffer_seconds > 0.0) || !std::isfinite(buffer_seconds)) bad("buffer_seconds", "must be finite and > 0");
  if (!(buffer_seconds >= window[1] - window[0])) bad("buffer_seconds", "must not be shorter than the window");
}

// ================================================================== the buffer
bool GyroBuffer::push(double t, const double w[3]) {
  if (!std::isfinite(t) || !std::isfinite(w[0]) || !std::isfinite(w[1]) || !std::isfinite(w[2]) || (!s_.empty() && !(t > s_.back().t))) {
    dropped_++;
    return false;
  }
  GyroSample g;
  g.t = t;
  for (int a = 0; a < 3; a++) g.w[a] = w[a];
  s_.push_back(g);
  while (!s_.empty() && s_.front().t < t - keep_) s_.pop_front();
  return true;
}

// ================================================================== samples -> table
std::optional<MotionTable> build_motion_table(const GyroBuffer& buffer, double timestamp, const GyroDeskewOptions& o, const double v[3]) {
  const auto& S = buffer.samples();
  const double lo = o.window[0], hi = o.window[1], t0 = timestamp + o.time_zero_offset;
  const uint32_t K = o.segments;
  // coverage: ia = the last sample at or before lo, ib = the first at or after hi
  long ia = -1, ib = -1;
  for (size_t j = 0; j < S.size(); j++) {
    const double tau = S[j].t - t0;
    if (tau <= lo) ia = (long)j;
    if (tau >= hi) { ib = (long)j; break; }
  }
  if (ia < 0 || ib < 0) return std::nullopt;
  const size_t n = (size_t)(ib - ia + 1);  // (>= 2: lo < hi)
  std::vector<double> tau(n);
  for (size_t j = 0; j < n; j++) tau[j] = S[(size_t)ia + j].t - t0;
  for (size_t j = 0; j + 1 < n; j++)
    if (tau[j + 1] - tau[j] > o.max_gap) return std::nullopt;
  auto W = [&](size_t j) { return S[(size_t)ia + j].w; };
  auto f = [&](double x, size_t j, double out[3]) {  // the interpolant on [tau_j, tau_j+1]
    const double u = (x - tau[j]) / (tau[j + 1] - tau[j]);
    for (int a = 0; a < 3; a++) out[a] = W(j)[a] + (W(j + 1)[a] - W(j)[a]) * u;
  };
  const double h = (hi - lo) / (double)K;
  MotionTable tab;
  tab.segments.resize(K);
  for (int a = 0; a < 3; a++) tab.v[a] = v[a];
  size_t j = 0;  // tau_j <= the current position (advances with the segments: the whole table is one walk over the samples)
  for (uint32_t s = 0; s < K; s++) {
    const double a0 = lo + (double)s * h, b0 = s + 1 < K ? lo + (double)(s + 1) * h : hi;
    while (j + 2 < n && tau[j + 1] <= a0) j++;
    double acc[3] = {0, 0, 0}, x0 = a0;
    size_t jj = j;
    while (x0 < b0) {
      const double x1 = std::min(b0, tau[jj + 1]);
      double f0[3], f1[3];
      f(x0, jj, f0);
      f(x1, jj, f1);
      for (int a = 0; a < 3; a++) acc[a] = acc[a] + 0.5 * (f0[a] + f1[a]) * (x1 - x0);
      x0 = x1;
      if (jj + 2 < n) jj++;
      else break;  // (the last sample interval reaches hi: x0 == b0 here)
    }
    mh_motion_segment& seg = tab.segments[s];
    seg.knot = a0;
    double m[3];
    for (int a = 0; a < 3; a++) m[a] = acc[a] / (b0 - a0) - o.gyro_bias[a];
    for (int a = 0; a < 3; a++) seg.w[a] = (o.sensor_rotation[a * 3] * m[0] + o.sensor_rotation[a * 3 + 1] * m[1]) + o.sensor_rotation[a * 3 + 2] * m[2];
  }
  // chain
  std::vector<double> A((size_t)K * 9);
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::copy(I, I + 9, A.begin());
  for (uint32_t s = 0; s + 1 < K; s++) {
    double E[9];
    exp_so3(tab.segments[s].w, h, E);
    mul33(&A[(size_t)s * 9], E, &A[(size_t)(s + 1) * 9]);
  }
  // anchor
  uint32_t cnt = 0;
  for (uint32_t s = 0; s < K; s++) cnt += tab.segments[s].knot <= 0.0 ? 1u : 0u;
  const uint32_t s0 = cnt ? std::min(cnt - 1, K - 1) : 0u;
  double E[9], Z[9], Zt[9];
  exp_so3(tab.segments[s0].w, 0.0 - tab.segments[s0].knot, E);
  mul33(&A[(size_t)s0 * 9], E, Z);
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) Zt[i * 3 + k] = Z[k * 3 + i];
  for (uint32_t s = 0; s < K; s++) mul33(Zt, &A[(size_t)s * 9], tab.segments[s].R);
  return tab;
}

// ================================================================== the text form
std::vector<GyroSample> parse_gyro_text(const std::string& text) {
  std::vector<GyroSample> out;
  std::istringstream in(text);
  std::string line;
  size_t no = 0;
  while (std::getline(in, line)) {
    no++;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    std::istringstream ls(line);
    std::vector<std::string> tok;
    for (std::string t; ls >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    if (tok.size() != 4) throw std::runtime_error("gyro file: line " + std::to_string(no) + ": expected 't wx wy wz', found " + std::to_string(tok.size()) + " fields");
    double val[4];
    for (int k = 0; k < 4; k++) {
      char* end = nullptr;
      val[k] = strtod(tok[(size_t)k].c_str(), &end);
      if (end == tok[(size_t)k].c_str() || *end != '\0' || !std::isfinite(val[k]))
        throw std::runtime_error("gyro file: line " + std::to_string(no) + ": '" + tok[(size_t)k] + "' is not a finite number");
    }
    GyroSample g;
    g.t = val[0];
    for (int a = 0; a < 3; a++) g.w[a] = val[1 + a];
    out.push_back(g);
  }
  return out;
}

std::vector<GyroSample> read_gyro_file(const std::string& path) { return parse_gyro_text(slurp("gyro file", path)); }

}  // namespace mola_hip
