// LoopClosure.h -- close the loops of a session and correct its key-frame poses: off-line on a recorded key-frame set (DESIGN.md
// section 0 row g6) and incrementally, one key-frame at a time, while driving (row g7).
//
// On a key-frame set (molahip_host/keyframe_file.h), with the device stages the relocalization already has:
//
//   per frame i   [device] describe layers[0] (mh_place_describe), search the descriptors of the other frames (mh_place_search)
//                 [host]   loop_candidates(): partners at least min_travel of path back, inside the position gate
//   per pair i,j  [device] the submap around j from its key-frames (insertFrames), the candidate grid around the recorded relative
//                          pose scored in one launch (mh_score_poses), the best few refined by the no-motion-model ICP
//                          (score_rank_refine of LidarOdometry.h: the relocalization's own step)
//                 [host]   accepted at min_quality: a loop edge Z_ji = frame i in frame j
//   once          [host]   optimize_pose_graph(): all frames, odometry edges from the recorded poses + the loop edges, fp64
//
// The corrected set differs from the input in its poses only, so build_session_maps() turns it into a consistent session map.
// Selection uses the recorded poses throughout.  close_loops() optimises once at the end.  The rule is causal -- frames in ascending
// order, a partner j < i, a submap of frames at least min_travel of path behind i -- so OnlineLoopCloser runs the same steps per
// pushed frame against a database that grows, optimises again from the raw chain with all loop edges so far whenever the set
// changes, and gives what close_loops() gives on the frames pushed so far, bit for bit; LidarOdometry feeds it and takes the
// correction back (online_loop_closure:).  Not here: online closure under an AlignBatcher, robust kernels or switchable
// constraints on loop edges, the recorded covariances as edge weights, several pairs verified as one lock-step batch, a batched
// descriptor self-join (one mh_place_search per frame instead: a batched one needs a new entry point), CVoxelMap plans.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/LidarOdometry.h"

namespace mola_hip {

// the optional top-level loop_closure: block of the pipeline file; an absent block gives the defaults
struct LoopClosureOptions {
  double min_travel = 30.0;                   // [m] a partner lies at least this much path length back
  double gate_base = 5.0, gate_rate = 0.02;   // position gate: |t_i - t_j| <= base + rate * (s_i - s_j)
  uint32_t max_place_dist = 0;                // bound on the descriptor distance; 0: off (the number is scene dependent)
  uint32_t top_k = 1;                         // eligible partners tried per frame, in rank order; the first accepted ends frame i
  double min_travel_between_closures = 10.0;  // [m] after an accepted closure at frame i, frames with s < s_i + this are skipped
  double submap_radius = 15.0;                // [m] of path around the partner
  double sigma_xy = 1.5, sigma_yaw_deg = 2.0;  // the candidate grid around the recorded relative pose
  double sigma = 0.0;                         // ADAPTIVE_THRESHOLD_SIGMA of the verification ICP (default: adaptive_threshold.initial_sigma)
  double min_quality = 0.9;                   // acceptance
  double odometry_sigma_xyz = 0.02, odometry_sigma_rot_deg = 0.05;  // weights of the edges between consecutive frames
  double loop_sigma_xyz = 0.05, loop_sigma_rot_deg = 0.1;           // ... and of the loop edges
  uint32_t max_iterations = 50;               // optimiser stop
  double min_step = 1e-9;
  // out of range (non-positive sigmas, top_k < 1, negative distances): std::runtime_error naming loop_closure: and the key
  static LoopClosureOptions FromConfig(const Config& pipeline);
  void validate() const;
};

// ---- candidate selection (host logic only: testable without a device)
struct LoopFrame {
  double pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  bool has_points = false;
  std::vector<PlaceIndex::Match> matches;  // as PlaceIndex returns them: (dist ascending, frame ascending), every frame of the index
};
struct LoopPair {
  uint32_t i = 0, j = 0, shift = 0, dist = 0;
};
// Path length s_0 = 0, s_k = s_{k-1} + |t_k - t_{k-1}| over all frames in order (frames without points included).  Frames i in
// ascending order; i is skipped when it has no points or s_i < s_c + min_travel_between_closures, c the last accepted closure's
// frame.  A partner j of i's match list is eligible when it has points, j < i, s_i - s_j >= min_travel, |t_i - t_j| <= gate_base +
// gate_rate * (s_i - s_j) and (max_place_dist == 0 or dist <= max_place_dist); both comparisons are closed.  The first top_k
// eligible partners in rank order are handed to `verify` one after another; the first it accepts ends frame i.  Returns every pair
// handed to verify, in that order.  verify == nullptr: every pair is accepted.
std::vector<LoopPair> loop_candidates(const std::vector<LoopFrame>& frames, const LoopClosureOptions& opt,
                                      const std::function<bool(const LoopPair&)>& verify = nullptr);
std::vector<double> path_lengths(const std::vector<LoopFrame>& frames);
// The rule for ONE frame i, which loop_candidates() folds over i = 0 .. K - 1: frames[0 .. i] and s[0 .. i] (their path lengths) are
// read, frames[i].matches may name later frames (they are skipped); `state` carries the last accepted closure's frame from step to
// step.  The pairs handed to verify are appended to `tried`; returns whether one was accepted.
struct LoopCandidateState {
  bool closed = false;    // a closure has been accepted ...
  double s_closed = 0.0;  // ... at this path length
};
bool loop_candidates_step(const std::vector<LoopFrame>& frames, const std::vector<double>& s, size_t i, const LoopClosureOptions& opt,
                          LoopCandidateState& state, const std::function<bool(const LoopPair&)>& verify, std::vector<LoopPair>& tried);

// ---- pose graph (host, fp64, no dependency)
struct PoseGraphEdge {
  uint32_t a = 0, b = 0;
  double Z[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // node b in node a
};
struct PoseGraphResult {
  std::vector<double> poses;  // 12 per node
  double cost_before = 0, cost_after = 0;
  uint32_t iterations = 0;
  std::vector<double> costs;  // the cost before the first step and after every accepted one: non-increasing
};
// Nodes: all poses (12 doubles each, row-major 3x4); node 0 is fixed and returned bit for bit.  Edges: (k - 1, k) with Z =
// T_{k-1}^-1 T_k from the given poses (weights 1 / odometry_sigma^2), and `loops` (weights 1 / loop_sigma^2).  Residual of an edge
// (a, b, Z): E = Z^-1 T_a^-1 T_b, r = [t(E); rotation vector of R(E)]; cost = sum r^T W r, W = diag(1 / sigma_xyz^2 x3, 1 /
// sigma_rot^2 x3).  Retraction T <- T [Exp_SO3(dtheta), dt].  Levenberg-Marquardt that starts undamped (a plain Gauss-Newton step;
// damping only after a step that would raise the cost) with analytic Jacobians; stops when max |delta| < min_step or after
// max_iterations.  Without loop edges the chain's residuals are zero by construction: the input is returned, cost 0, 0 iterations.
// Linear solve: a profile (envelope) Cholesky of the 6 (K - 1) normal equations in node order -- a row's envelope starts at the
// lowest node it shares an edge with, fill stays inside it, no dense matrix is formed.  Memory 36 (K + sum of the loops' spans)
// doubles, time O(6^3 (K + sum of spans)) per iteration while the loops' spans do not nest deeply (a row whose envelope overlaps
// w rows of other loops pays w times).  A loop edge that names a node >= K, or a == b: std::runtime_error.
PoseGraphResult optimize_pose_graph(const std::vector<double>& poses, const std::vector<PoseGraphEdge>& loops, const LoopClosureOptions& opt);

// ---- the whole thing
struct LoopReport {
  struct Pair {
    uint32_t i = 0, j = 0, shift = 0, dist = 0, candidates = 0, iterations = 0;
    std::vector<uint32_t> ranks;  // the candidates refined, in rank order
    double quality = 0;
    bool accepted = false;
    double Z[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // the winner: frame i in frame j
  };
  std::vector<Pair> pairs;
  double cost_before = 0, cost_after = 0;
  uint32_t optimizer_iterations = 0;
  std::map<std::string, double> seconds;  // wall time per stage: describe, search, submap, score, refine, optimize
  std::map<std::string, double> counts;   // calls per stage
  std::string toJson() const;
};
struct LoopClosureResult {
  molahip_host::KeyFrameSet corrected;  // the input with other poses; without an accepted loop the input, bit for bit
  LoopReport report;
};
// `pipeline`: the whole pipeline file (icp_settings_without_vel or icp_settings_with_vel, params, relocalization:, loop_closure:).
// Every (global, local) entry of every enabled matcher must name a target map of the set's header as its global layer
// (std::runtime_error naming it otherwise); a header with a CVoxelMap is refused as build_session_maps refuses it.
LoopClosureResult close_loops(const molahip_host::KeyFrameSet& set, const Config& pipeline, std::shared_ptr<DeviceContext> ctx = nullptr);
// ... file to file: reads `keyframe_file`, writes the corrected set to `output_keyframe_file` (a version-1 key-frame file)
LoopReport close_loops_file(const std::string& keyframe_file, const Config& pipeline, const std::string& output_keyframe_file,
                            std::shared_ptr<DeviceContext> ctx = nullptr);


// ---- while driving
// the optional top-level online_loop_closure: block (this implementation's own key); the gates, the grid, the weights and the
// acceptance are the loop_closure: block's
struct OnlineLoopClosureOptions {
  bool enabled = false;                  // off: nothing of this runs
  bool correct_driver = true;            // LidarOdometry: feed an accepted closure back into pose, motion model, key-frames and local maps
  uint32_t check_every_n_keyframes = 1;  // frames with points are described and added every time; candidates are looked for on every n-th
  // out of range: std::runtime_error naming online_loop_closure: and the key
  static OnlineLoopClosureOptions FromConfig(const Config& pipeline);
  void validate() const;
};

// The ICP block a loop closure verifies with must match against the target maps: every (global, local) entry of every enabled
// matcher names one of `map_names` as its global layer, a local layer goes to one map only, and there is an enabled
// Matcher_Points_DistanceThreshold to score candidates with.  Throws std::runtime_error("<who>: ...") otherwise (close_loops'
// texts); needs no device.
void check_loop_closure_icp(ICP& icp, const std::vector<std::string>& map_names, const std::string& who);

// The incremental form of close_loops(): push() takes the stored frames of a drive one by one, in order, each with its RAW pose --
// the chain as it was estimated, which no correction ever touches; selection and verification work on it as the off-line form works
// on the recorded poses.  Frame i is described once, searched against the descriptors of the frames < i that have points, then
// added; the candidate rule is loop_candidates_step() with the carried state, verification is close_loops' own.  Whenever loop edges
// exist the corrected poses are optimize_pose_graph(rawPoses(), loops()) from scratch, never from the previous correction.  So after
// pushing frames 0 .. i, report().pairs (every field, Z included) and correctedPoses() are what close_loops() returns for the set
// {maps, frames 0 .. i}, bit for bit (for min_travel > 0; at 0 the off-line submap may hold frame i's successors at its very
// position).  With check_every_n_keyframes = n only every n-th frame with points (the first, the (n + 1)-th, ...) is searched and
// handed to the candidate rule: the tried pairs are then the fold of loop_candidates_step() over those frames.
// report(): the stage names and counts of the off-line report; "optimize" counts one per accepted closure (its seconds include the
// re-optimisations that carry the correction to the frames pushed after it), cost_* and optimizer_iterations are the last one's.
// The frames' layers are kept (a verification builds its submap from them) unless readFramesFrom() names the caller's copy.  Throws
// what close_loops() throws, named OnlineLoopCloser; a push that throws leaves the closer as it was before it.
struct LoopCloserCore;  // what both forms share (loop_closure.cpp)
class OnlineLoopCloser {
 public:
  struct Step {
    bool tried = false, closed = false;
    std::vector<LoopReport::Pair> pairs;  // the pairs verified for this frame, in order
  };
  OnlineLoopCloser(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, std::shared_ptr<DeviceContext> ctx = nullptr);
  ~OnlineLoopCloser();
  OnlineLoopCloser(const OnlineLoopCloser&) = delete;
  OnlineLoopCloser& operator=(const OnlineLoopCloser&) = delete;
  Step push(molahip_host::KeyFrame frame_with_raw_pose);  // one stored frame, with or without points; the closer keeps it (move it in)
  // A caller that holds the frames itself (the driver's key-frame store): `frames` is read by index instead -- layers only, the
  // poses it holds are never looked at -- and the closer keeps no copy of the points.  Before the first push; the vector must
  // outlive the closer, keep frame k at index k and leave the layers of pushed frames alone.  Then pushStored(k, raw pose) takes
  // frame k = size() of that vector.
  void readFramesFrom(const std::vector<molahip_host::KeyFrame>* frames);
  Step pushStored(size_t index, const double raw_pose[12]);
  size_t size() const;
  const std::vector<double>& rawPoses() const;        // 12 per frame
  const std::vector<double>& correctedPoses() const;  // == rawPoses() until the first accepted loop
  const std::vector<PoseGraphEdge>& loops() const;
  const LoopReport& report() const;
  const OnlineLoopClosureOptions& options() const { return online_; }
  molahip_host::KeyFrameSet rawKeyFrames() const;  // the frames as pushed, under `maps`: the input on which close_loops() reproduces this

 private:
  std::unique_ptr<LoopCloserCore> core_;
  OnlineLoopClosureOptions online_;
  LoopCandidateState state_;
  Step push_frame(const molahip_host::KeyFrame& frame, const double raw_pose[12]);
  std::vector<molahip_host::KeyFrame> frames_;                     // the pushed frames ...
  const std::vector<molahip_host::KeyFrame>* external_ = nullptr;  // ... or the caller's (readFramesFrom)
  std::vector<double> raw_, corrected_;
  size_t n_with_points_ = 0;
};

}  // namespace mola_hip
