// GyroDeskew.h -- de-skew with gyroscope samples: the host rule that turns the samples of a sweep into the piecewise motion
// table of include/molahip_motion.h.  Host logic only, all of it fp64; tests/motion_ref.py restates it.
//
// FilterDeskew assumes one constant twist over the sweep, taken from the last two registered poses.  Where the rotation rate
// changes inside a sweep no such twist describes it; a gyroscope measures exactly that rate.  The optional top-level block
// gyro_deskew: (this implementation's own key) makes the odometry driver de-skew with the measured rotation:
//
//   gyro_deskew:
//     enabled: false
//     window: [-0.06, 0.06]     # [s] the span of the point stamps the table covers, relative to the scan's zero; lo < hi
//     segments: 12              # K, 1 .. 64 (MH_MOTION_MAX_SEGMENTS)
//     max_gap: 0.02             # [s] the largest step between consecutive samples inside the window
//     time_zero_offset: 0       # [s] the absolute time of a point is  timestamp + time_zero_offset + t_i
//     gyro_bias: [0, 0, 0]      # [rad/s] subtracted from every sample, sensor frame
//     sensor_rotation: [1, 0, 0, 0, 1, 0, 0, 0, 1]   # row-major, from the gyro's frame to the vehicle's (orthonormal to 1e-6)
//     buffer_seconds: 2         # samples older than the newest by more than this are forgotten
//
// THE RULE, build_motion_table(buffer, timestamp, options, v).  tau_j = t_j - (timestamp + time_zero_offset) are the sample
// times on the axis of the point stamps; f(tau) is the linear interpolant of the samples.
//   - knots:    k_s = lo + s h, h = (hi - lo) / K, s = 0 .. K-1; the upper end of segment s is k_{s+1}, of the last one hi.
//   - rate:     m_s = the mean of f over the segment -- the exact integral of a piecewise-linear function, piece by piece between
//               the segment's ends and the samples inside it, (f(x0) + f(x1)) / 2 * (x1 - x0) each, divided by the segment's
//               length; w_s = sensor_rotation * (m_s - gyro_bias).
//   - chain:    A_0 = I, A_{s+1} = A_s Exp_SO3(w_s h).
//   - anchor:   s0 = the device rule's segment for t = 0 (clamp(#{k_s <= 0} - 1, 0, K-1)), Z = A_{s0} Exp_SO3(w_{s0} (0 - k_{s0}));
//               R_s = Z^T A_s: the rotation at t = 0 is the identity, as FilterDeskew's is.
//   - coverage: a sample at or before lo (the last such one starts the interpolant), a sample at or after hi (the first such one
//               ends it), and no step above max_gap between consecutive samples from the one to the other.  Otherwise: no table
//               (the driver then de-skews that scan with the constant twist).
//   Only the rotation comes from the gyro; `v` is handed through (the motion model's, then the twist hook's).
#pragma once
#include <cstdint>
#include <deque>
#include <optional>
#include <vector>

#include "molahip_motion.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

struct GyroDeskewOptions {
  bool enabled = false;
  double window[2] = {-0.06, 0.06};
  uint32_t segments = 12;
  double max_gap = 0.02;
  double time_zero_offset = 0.0;
  double gyro_bias[3] = {0, 0, 0};
  double sensor_rotation[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double buffer_seconds = 2.0;
  // the gyro_deskew: block of a pipeline (absent: the defaults); out of range or an unknown key: std::runtime_error starting
  // "gyro_deskew: <key>"
  static GyroDeskewOptions FromConfig(const mp2p_icp_hip::Config& pipeline);
  void validate() const;
};

struct GyroSample {
  double t = 0;  // absolute [s], the clock of the scans' time stamps
  double w[3] = {0, 0, 0};  // [rad/s], the gyro's frame
};

// The samples in strictly increasing time.  A sample whose time does not increase -- or that is not finite -- is dropped and counted.
class GyroBuffer {
 public:
  explicit GyroBuffer(double buffer_seconds = 2.0) : keep_(buffer_seconds) {}
  bool push(double t, const double w[3]);  // false: dropped
  void clear() { s_.clear(); dropped_ = 0; }
  void setBufferSeconds(double s) { keep_ = s; }
  const std::deque<GyroSample>& samples() const { return s_; }
  size_t size() const { return s_.size(); }
  uint64_t dropped() const { return dropped_; }

 private:
  std::deque<GyroSample> s_;
  double keep_;
  uint64_t dropped_ = 0;
};

// a table that owns its segments; table() is the view the C ABI takes (valid while this object lives and is not changed)
struct MotionTable {
  std::vector<mh_motion_segment> segments;
  double v[3] = {0, 0, 0};
  mh_motion_table table() const {
    mh_motion_table t;
    t.n_segments = (uint32_t)segments.size();
    t.reserved_ = 0;
    t.segments = segments.data();
    for (int a = 0; a < 3; a++) t.v[a] = v[a];
    return t;
  }
};

std::optional<MotionTable> build_motion_table(const GyroBuffer& buffer, double timestamp, const GyroDeskewOptions& options, const double v[3]);

// the text form the command line reads: lines "t wx wy wz", '#' starts a comment, blank lines allowed; anything else:
// std::runtime_error naming the line
std::vector<GyroSample> parse_gyro_text(const std::string& text);
std::vector<GyroSample> read_gyro_file(const std::string& path);

}  // namespace mola_hip
