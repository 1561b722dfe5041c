// SessionJoin.h -- two recorded sessions put into one frame: one key-frame set, and through build_session_maps() one map (DESIGN.md
// section 0 row g8).  Beside LoopClosure.h, with its device stages and nothing else:
//
//   once          [device] the descriptors of A's frames into a PlaceIndex (ONE addKeyFrames: one mh_place_db_add_frames)
//   per B frame   [device] describe layers[0], search A's descriptors (PlaceIndex::query: mh_place_describe + mh_place_search)
//   per pair b,j  [device] the submap around A's frame j (insertFrames), the candidate grid scored in one launch (mh_score_poses), the
//                          best few refined by the no-motion-model ICP (score_rank_refine): close_loops' verification, on another
//                          grid centre
//   once          [host]   optimize_pose_graph_anchored(): A fixed, B's chain, one edge per accepted link
//
// THE RULE.  A's frames keep their poses TA; B's poses TB are in B's own frame, which has nothing to do with A's.  sB =
// path_lengths over B.  Poses compose as CPose3D does: X + Y is X (+) Y, X - Y is Y^-1 (+) X.
//   1. Index.  The descriptors of all A frames with points go in by one PlaceIndex::addKeyFrames.  Each B frame with points is
//      queried once; its match list is ranked (dist, frame) ascending and names A's frames.
//   2. Anchor.  B's frames with points are visited in ascending order, at most max_anchor_frames of them (0: all).  The partners of
//      frame b are the first top_k entries of its match list that have points and pass max_place_dist (0: off; the comparison is
//      closed).  Each pair (b, j) is verified as close_loops verifies a pair -- the submap is A's frames with points within
//      submap_radius of path of j (no causality condition), acceptance is at loop_closure.min_quality -- around the guess
//      relocalizeInKeyFrames makes: the centre is Rz(-shift * 2 pi / place_sectors) with zero translation, the grid is
//      relocalization.place_sigma_xy / place_sigma_yaw_deg.  The first accepted pair (b*, j*, Z*) is the anchor.  Without one:
//      is_joined = false, `joined` is A, the report lists the pairs tried.
//   3. Links.  Two sweeps start from b*: forward over b* + 1 .. KB - 1, then backward over b* - 1 .. 0.  Each carries the last
//      accepted link (b', j', Z'); both start with the anchor.  Frame b is skipped when it has no points or |sB_b - sB_b'| <
//      min_travel_between_links.  Its predicted pose in A's frame is P_b = (TA_j' + Z') + (TB_b - TB_b').  A partner j of b's match
//      list is eligible when it has points, passes max_place_dist, and |t(P_b) - t(TA_j)| <= gate_base + gate_rate * |sB_b - sB_b'|
//      (closed).  The first top_k eligible partners are verified in rank order around the centre P_b - TA_j on the loop_closure:
//      grid (sigma_xy, sigma_yaw_deg).  The first accepted pair ends the frame and becomes the sweep's carried link.
//   4. Decision.  is_joined = the number of accepted links, the anchor included, is >= min_links; otherwise `joined` is A.  A wrong
//      anchor predicts wrong places, so it finds no second link: that is what the default min_links = 2 is for.  With min_links =
//      1 a single descriptor coincidence that the ICP happens to accept joins the sessions.
//   5. Poses.  A is fixed and returned bit for bit.  optimize_pose_graph_anchored() over A's nodes then B's, B's chain starting at
//      node KA, one edge (A_j, KA + b, Z) per accepted link in the order they were accepted -- the anchor first, so B starts at
//      T_AB + TB_b, T_AB = (TA_j* + Z*) + TB_b*^-1.
//   6. Output.  The header is A's; the frames are A's, then B's with the new poses -- timestamps, covariances, twists and layers
//      untouched.  A version-1 key-frame file: build_session_maps() and close_loops() take it as it is.
//
// Not here: A is never moved (its own drift stays; so does every map built from it); no loops inside B (run close_loops on the
// result); more than two sessions go in by repeated joins; no robust kernel or switchable constraint on the links; CVoxelMap plans;
// several pairs verified as one lock-step batch.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/LoopClosure.h"

namespace mola_hip {

// the optional top-level session_join: block of the pipeline file (this implementation's own key); an absent block gives the
// defaults.  The gates, the submap, the grids, the acceptance, the weights and the optimiser's stops are read from loop_closure:
// (gate_base, gate_rate, submap_radius, sigma_xy, sigma_yaw_deg, sigma, min_quality, odometry_sigma_*, loop_sigma_*,
// max_iterations, min_step), the descriptor, the anchor's grid and the scoring from relocalization: (place_*, score_threshold,
// step_*, sigmas, refine_top_k, max_candidates).
struct SessionJoinOptions {
  uint32_t top_k = 0;                      // partners tried per frame, in rank order; 0: relocalization.place_top_k
  uint32_t max_place_dist = 0;             // bound on the descriptor distance; 0: off
  uint32_t min_links = 2;                  // accepted links (the anchor counts) needed to call the sessions joined
  double min_travel_between_links = 10.0;  // [m] of B's path between a link and the next frame tried
  uint32_t max_anchor_frames = 0;          // B frames (with points) tried for the anchor; 0: all
  // out of range (min_links < 1, a negative or non-finite distance, a count that is no integer >= 0): std::runtime_error naming
  // session_join: and the key
  static SessionJoinOptions FromConfig(const Config& pipeline);
  void validate() const;
};

// ---- candidate selection (host logic only: testable without a device)
enum JoinPhase : uint32_t { JOIN_ANCHOR = 0, JOIN_FORWARD = 1, JOIN_BACKWARD = 2 };
struct JoinPair {
  uint32_t b = 0, j = 0, shift = 0, dist = 0;  // B's frame, A's frame, the match
  uint32_t phase = JOIN_ANCHOR;
  double centre[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // the guess of B's frame b in A's frame j the grid is laid around
};
struct JoinLink {  // an accepted pair: Z = B's frame b in A's frame j
  uint32_t b = 0, j = 0;
  double Z[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
};
// hands a pair to the verification; true: accepted, and Z is written
using JoinVerify = std::function<bool(const JoinPair&, double Z[12])>;
// nullptr as `verify` below: every pair is accepted with Z = its centre.
//
// Step 2 for ONE frame b of B (A's frames: pose and has_points are read; B's: has_points and matches, which name A's frames;
// place_sectors: relocalization.place_sectors).  `top_k` here and below is the resolved one (>= 1).  The pairs handed to verify are
// appended to `tried`; returns whether one was accepted, then `anchor` holds it.
bool join_anchor_step(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, size_t b, uint32_t top_k, uint32_t max_place_dist,
                      uint32_t place_sectors, const JoinVerify& verify, std::vector<JoinPair>& tried, JoinLink& anchor);
// Step 3 for ONE frame b of a sweep (`phase`: JOIN_FORWARD or JOIN_BACKWARD; sB: B's path lengths): `carried` is the sweep's last
// accepted link and is replaced when b is accepted.  gate_base and gate_rate are read from `gates`.
bool join_candidates_step(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, const std::vector<double>& sB, size_t b, uint32_t phase,
                          const SessionJoinOptions& opt, uint32_t top_k, const LoopClosureOptions& gates, JoinLink& carried, const JoinVerify& verify,
                          std::vector<JoinPair>& tried);
// Steps 2 and 3 folded over B: every pair handed to verify, in order, and the accepted links (the anchor first, then the forward
// sweep's, then the backward sweep's).
struct JoinCandidates {
  std::vector<JoinPair> tried;
  std::vector<JoinLink> links;
};
JoinCandidates join_candidates(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, const SessionJoinOptions& opt, uint32_t top_k,
                               uint32_t place_sectors, const LoopClosureOptions& gates, const JoinVerify& verify = nullptr);

// ---- pose graph with fixed nodes (host, fp64; residual, retraction, Levenberg-Marquardt schedule and envelope Cholesky are
// optimize_pose_graph's, LoopClosure.h)
// Nodes: all poses (12 doubles each); the first n_fixed (>= 1) are fixed and returned bit for bit.  The free nodes form chains: a
// chain starts at node n_fixed and at every node of `chain_starts`; inside a chain there is an edge (k - 1, k) with Z = T_{k-1}^-1
// T_k from the given poses (odometry weights).  `edges` (loop weights) each join a fixed node and a free one, or two free ones; an
// edge between two fixed nodes, to itself, or naming a node that is not there: std::runtime_error.  A chain's given poses may be in
// any frame: before anything else a chain is placed rigidly by its first edge from a fixed node in `edges` order, T_k <- G + T_k
// with G = (T_a + Z) + T_b^-1 for an edge (a fixed, b in the chain) and G = (T_b + Z^-1) + T_a^-1 for one given backwards.  A chain
// without an edge from a fixed node: std::runtime_error (its frame is undetermined).  When no chain has more than one edge and every edge comes from a fixed node, all residuals are zero by construction:
// the placement is returned, cost 0, 0 iterations.  An edge to a fixed node adds no span to the envelope.
PoseGraphResult optimize_pose_graph_anchored(const std::vector<double>& poses, size_t n_fixed, const std::vector<uint32_t>& chain_starts,
                                             const std::vector<PoseGraphEdge>& edges, const LoopClosureOptions& opt);

// ---- the whole thing
struct SessionJoinReport {
  struct Pair : LoopReport::Pair {  // i: B's frame, j: A's frame, Z: B's frame i in A's frame j
    uint32_t phase = JOIN_ANCHOR;
  };
  std::vector<Pair> pairs;
  uint32_t links_accepted = 0;
  bool joined = false;
  double cost_before = 0, cost_after = 0;
  uint32_t optimizer_iterations = 0;
  std::map<std::string, double> seconds;  // wall time per stage: index, search, submap, score, refine, optimize
  std::map<std::string, double> counts;   // calls per stage
  std::string toJson() const;
};
struct SessionJoinResult {
  molahip_host::KeyFrameSet joined;  // A's frames bit for bit, then B's with their poses in A's frame; A alone when !is_joined
  bool is_joined = false;
  SessionJoinReport report;
};
// `pipeline`: the whole pipeline file, as close_loops takes it.  B's header must name A's target maps -- names, classes and
// parameters, in order -- else std::runtime_error naming the first difference; a header with a CVoxelMap is refused as
// build_session_maps refuses it; the ICP block is held to check_loop_closure_icp.  An empty B, or one without a frame with points,
// is not joined.
SessionJoinResult join_sessions(const molahip_host::KeyFrameSet& A, const molahip_host::KeyFrameSet& B, const Config& pipeline,
                                std::shared_ptr<DeviceContext> ctx = nullptr);
// ... file to file: the joined set is written to `output_keyframe_file` (a version-1 key-frame file) when the sessions are joined,
// nothing is written when they are not
SessionJoinReport join_sessions_file(const std::string& keyframe_file_a, const std::string& keyframe_file_b, const Config& pipeline,
                                     const std::string& output_keyframe_file, std::shared_ptr<DeviceContext> ctx = nullptr);

}  // namespace mola_hip
