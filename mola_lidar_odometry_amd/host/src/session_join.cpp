// session_join.cpp -- see mola_lidar_odometry_hip/SessionJoin.h.  Host logic only: the device is reached through PlaceIndex and the
// pair verification of loop_closure.cpp; the optimiser with fixed nodes lives there too, beside the one it shares its loop with.
#include "mola_lidar_odometry_hip/SessionJoin.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "loop_closure_internal.h"

namespace mola_hip {

using namespace mp2p_icp_hip;

namespace {

CPose3D pose_of(const double* T) {
  CPose3D p;
  std::copy(T, T + 12, p.T);
  return p;
}

double distance(const double* a, const double* b) {  // |t_b - t_a|
  const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
  return std::sqrt(dx * dx + dy * dy + dz * dz);
}

struct Timer {  // adds the wall time of its scope to a report entry, and one to its call count
  SessionJoinReport& r;
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  Timer(SessionJoinReport& rep, const char* n) : r(rep), name(n) { r.counts[n] += 1.0; }
  ~Timer() { r.seconds[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace

// ================================================================== options
SessionJoinOptions SessionJoinOptions::FromConfig(const Config& cfg) {
  SessionJoinOptions o;
  if (cfg.has("session_join") && !cfg["session_join"].isNull()) {
    const Config& c = cfg["session_join"];
    auto cnt = [&](const char* k, uint32_t& v, double least) {
      if (!c.has(k) || c[k].isNull()) return;
      const double d = strtod(c[k].asString().c_str(), nullptr);
      if (!(d >= least) || !(d <= 4294967295.0) || d != std::floor(d))
        throw std::runtime_error(std::string("session_join: ") + k + " must be an integer >= " + std::to_string((int)least));
      v = (uint32_t)d;
    };
    cnt("top_k", o.top_k, 0.0);
    cnt("max_place_dist", o.max_place_dist, 0.0);
    cnt("min_links", o.min_links, 1.0);
    if (c.has("min_travel_between_links") && !c["min_travel_between_links"].isNull())
      o.min_travel_between_links = strtod(c["min_travel_between_links"].asString().c_str(), nullptr);
    cnt("max_anchor_frames", o.max_anchor_frames, 0.0);
  }
  o.validate();
  return o;
}

void SessionJoinOptions::validate() const {
  if (min_links < 1) throw std::runtime_error("session_join: min_links must be an integer >= 1");
  if (!(min_travel_between_links >= 0.0) || !std::isfinite(min_travel_between_links))
    throw std::runtime_error("session_join: min_travel_between_links must be finite and >= 0");
}

// ================================================================== candidate selection
namespace {
bool hand_over(JoinPair& p, const CPose3D& centre, const JoinVerify& verify, std::vector<JoinPair>& tried, JoinLink& link) {
  std::copy(centre.T, centre.T + 12, p.centre);
  tried.push_back(p);
  double Z[12];
  std::copy(p.centre, p.centre + 12, Z);
  if (verify && !verify(p, Z)) return false;
  link.b = p.b; link.j = p.j;
  std::copy(Z, Z + 12, link.Z);
  return true;
}
}  // namespace

bool join_anchor_step(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, size_t b, uint32_t top_k, uint32_t max_place_dist,
                      uint32_t place_sectors, const JoinVerify& verify, std::vector<JoinPair>& tried, JoinLink& anchor) {
  if (!B[b].has_points) return false;
  uint32_t n = 0;
  for (const PlaceIndex::Match& m : B[b].matches) {
    if (n >= top_k) break;
    if (m.frame >= A.size() || !A[m.frame].has_points) continue;
    if (max_place_dist != 0 && m.dist > max_place_dist) continue;
    n++;
    JoinPair p;
    p.b = (uint32_t)b; p.j = m.frame; p.shift = m.shift; p.dist = m.dist; p.phase = JOIN_ANCHOR;
    TPose3D rz;
    rz.yaw = -(double)m.shift * 2.0 * M_PI / (double)place_sectors;
    if (hand_over(p, CPose3D(rz), verify, tried, anchor)) return true;
  }
  return false;
}

bool join_candidates_step(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, const std::vector<double>& sB, size_t b, uint32_t phase,
                          const SessionJoinOptions& opt, uint32_t top_k, const LoopClosureOptions& gates, JoinLink& carried, const JoinVerify& verify,
                          std::vector<JoinPair>& tried) {
  if (!B[b].has_points) return false;
  const double travel = std::fabs(sB[b] - sB[carried.b]);
  if (travel < opt.min_travel_between_links) return false;
  const CPose3D P = (pose_of(A[carried.j].pose) + pose_of(carried.Z)) + (pose_of(B[b].pose) - pose_of(B[carried.b].pose));
  uint32_t n = 0;
  for (const PlaceIndex::Match& m : B[b].matches) {
    if (n >= top_k) break;
    if (m.frame >= A.size() || !A[m.frame].has_points) continue;
    if (opt.max_place_dist != 0 && m.dist > opt.max_place_dist) continue;
    if (!(distance(A[m.frame].pose, P.T) <= gates.gate_base + gates.gate_rate * travel)) continue;
    n++;
    JoinPair p;
    p.b = (uint32_t)b; p.j = m.frame; p.shift = m.shift; p.dist = m.dist; p.phase = phase;
    if (hand_over(p, P - pose_of(A[m.frame].pose), verify, tried, carried)) return true;
  }
  return false;
}

JoinCandidates join_candidates(const std::vector<LoopFrame>& A, const std::vector<LoopFrame>& B, const SessionJoinOptions& opt, uint32_t top_k,
                               uint32_t place_sectors, const LoopClosureOptions& gates, const JoinVerify& verify) {
  if (top_k < 1) throw std::runtime_error("join_candidates: top_k must be resolved (>= 1)");
  if (place_sectors < 1) throw std::runtime_error("join_candidates: place_sectors must be >= 1");
  JoinCandidates out;
  const std::vector<double> sB = path_lengths(B);
  JoinLink anchor;
  bool have = false;
  uint32_t visited = 0;
  for (size_t b = 0; b < B.size() && !have; b++) {
    if (!B[b].has_points) continue;
    if (opt.max_anchor_frames != 0 && visited >= opt.max_anchor_frames) break;
    visited++;
    have = join_anchor_step(A, B, b, top_k, opt.max_place_dist, place_sectors, verify, out.tried, anchor);
  }
  if (!have) return out;
  out.links.push_back(anchor);
  JoinLink carried = anchor;
  for (size_t b = anchor.b + 1; b < B.size(); b++)
    if (join_candidates_step(A, B, sB, b, JOIN_FORWARD, opt, top_k, gates, carried, verify, out.tried)) out.links.push_back(carried);
  carried = anchor;
  for (size_t b = anchor.b; b-- > 0;)
    if (join_candidates_step(A, B, sB, b, JOIN_BACKWARD, opt, top_k, gates, carried, verify, out.tried)) out.links.push_back(carried);
  return out;
}

// ================================================================== report
std::string SessionJoinReport::toJson() const {
  std::string o = "{\"pairs\": [";
  char buf[64];
  auto num = [&](double v) {
    snprintf(buf, sizeof(buf), "%.17g", v);
    return std::string(std::isfinite(v) ? buf : "null");
  };
  static const char* const phases[3] = {"anchor", "forward", "backward"};
  for (size_t k = 0; k < pairs.size(); k++) {
    const Pair& p = pairs[k];
    o += std::string(k ? ", " : "") + "{\"i\": " + std::to_string(p.i) + ", \"j\": " + std::to_string(p.j) + ", \"phase\": \"" + phases[std::min(p.phase, 2u)] +
         "\", \"shift\": " + std::to_string(p.shift) + ", \"dist\": " + std::to_string(p.dist) + ", \"candidates\": " + std::to_string(p.candidates) +
         ", \"ranks\": [";
    for (size_t c = 0; c < p.ranks.size(); c++) o += (c ? ", " : "") + std::to_string(p.ranks[c]);
    o += "], \"quality\": " + num(p.quality) + ", \"iterations\": " + std::to_string(p.iterations) + ", \"accepted\": " + (p.accepted ? "true" : "false") +
         ", \"Z\": [";
    for (int c = 0; c < 12; c++) o += (c ? ", " : "") + num(p.Z[c]);
    o += "]}";
  }
  o += "], \"links_accepted\": " + std::to_string(links_accepted) + ", \"joined\": " + (joined ? "true" : "false") + ", \"cost_before\": " + num(cost_before) +
       ", \"cost_after\": " + num(cost_after) + ", \"optimizer_iterations\": " + std::to_string(optimizer_iterations);
  auto table = [&](const char* name, const std::map<std::string, double>& m) {
    o += std::string(", \"") + name + "\": {";
    bool firstEntry = true;
    for (const auto& kv : m) {
      o += std::string(firstEntry ? "" : ", ") + "\"" + kv.first + "\": " + num(kv.second);
      firstEntry = false;
    }
    o += "}";
  };
  table("seconds", seconds);
  table("counts", counts);
  o += "}\n";
  return o;
}

// ================================================================== join_sessions
namespace {
void same_headers(const std::vector<molahip_host::KeyFrameTarget>& a, const std::vector<molahip_host::KeyFrameTarget>& b) {
  const std::string who = "join_sessions: the two key-frame files were not recorded for the same target maps: ";
  if (a.size() != b.size()) throw std::runtime_error(who + "the first names " + std::to_string(a.size()) + ", the second " + std::to_string(b.size()));
  for (size_t k = 0; k < a.size(); k++) {
    const std::string m = "map " + std::to_string(k) + " ";
    if (a[k].name != b[k].name) throw std::runtime_error(who + m + "is '" + a[k].name + "' in the first and '" + b[k].name + "' in the second");
    if (a[k].class_name != b[k].class_name)
      throw std::runtime_error(who + m + "('" + a[k].name + "') is a '" + a[k].class_name + "' in the first and a '" + b[k].class_name + "' in the second");
    const mh_map_params &p = a[k].params, &q = b[k].params;
    auto differ = [&](const char* field, double x, double y) {
      if (x != y) throw std::runtime_error(who + m + "('" + a[k].name + "') has " + field + " " + std::to_string(x) + " in the first and " + std::to_string(y) + " in the second");
    };
    differ("voxel_size", p.voxel_size, q.voxel_size);
    differ("max_points_per_voxel", p.max_points_per_voxel, q.max_points_per_voxel);
    differ("index_mode", p.index_mode, q.index_mode);
    differ("min_distance_between_points", p.min_distance_between_points, q.min_distance_between_points);
    differ("ndt_max_eigen_ratio", p.ndt_max_eigen_ratio, q.ndt_max_eigen_ratio);
    differ("ndt_min_points", p.ndt_min_points, q.ndt_min_points);
    differ("far_voxel_metric", p.far_voxel_metric, q.far_voxel_metric);
    differ("remove_voxels_farther_than", a[k].remove_voxels_farther_than, b[k].remove_voxels_farther_than);
  }
}
}  // namespace

SessionJoinResult join_sessions(const molahip_host::KeyFrameSet& A, const molahip_host::KeyFrameSet& B, const Config& pipeline,
                                std::shared_ptr<DeviceContext> ctx) {
  const SessionJoinOptions jopt = SessionJoinOptions::FromConfig(pipeline);
  same_headers(A.maps, B.maps);
  for (const molahip_host::KeyFrameSet* set : {&A, &B})
    for (const auto& f : set->frames)
      for (int k = 0; k < 12; k++)
        if (!std::isfinite(f.pose[k])) throw std::runtime_error("join_sessions: non-finite pose");
  PairVerifier::checkWithoutDevice(A.maps, pipeline, "join_sessions");
  SessionJoinResult out;
  out.joined = A;
  SessionJoinReport& rep = out.report;
  const size_t KA = A.frames.size(), KB = B.frames.size();
  std::vector<LoopFrame> fb(KB);
  bool any_a = false, any_b = false;
  for (size_t b = 0; b < KB; b++) {
    std::copy(B.frames[b].pose, B.frames[b].pose + 12, fb[b].pose);
    fb[b].has_points = PairVerifier::usable(B.frames[b]);
    any_b = any_b || fb[b].has_points;
  }
  for (const auto& f : A.frames) any_a = any_a || PairVerifier::usable(f);
  if (!any_a || !any_b) return out;  // nothing to describe on one side: not joined, and no device is asked for
  PairVerifier pv(A.maps, pipeline, std::move(ctx), "join_sessions");
  const LoopClosureOptions& lopt = pv.options();
  const LidarOdometry::RelocalizationOptions& reloc = pv.relocalization();
  const uint32_t top_k = jopt.top_k != 0 ? jopt.top_k : std::max<uint32_t>(reloc.place_top_k, 1);
  pv.setMapFrames(A.frames);

  // ---- 1. the index over A, B's match lists
  PlaceIndex index(pv.placeParams(), pv.context());
  {
    Timer t(rep, "index");
    index.addKeyFrames(A);
  }
  for (size_t b = 0; b < KB; b++) {
    if (!fb[b].has_points) continue;
    Timer t(rep, "search");
    const auto& l = B.frames[b].layers[0];
    DevicePointCloud layer(pv.context());
    layer.setPoints(l.x.data(), l.y.data(), l.z.data(), l.x.size());
    fb[b].matches = index.query(layer);
  }

  // ---- 2-4. anchor, links, decision
  const double place_yaw = reloc.place_sigma_yaw_deg;
  const JoinVerify verify = [&](const JoinPair& p, double Z[12]) {
    SessionJoinReport::Pair pr;
    pr.i = p.b; pr.j = p.j; pr.shift = p.shift; pr.dist = p.dist; pr.phase = p.phase;
    const bool anchor = p.phase == JOIN_ANCHOR;
    pv.verify(B.frames[p.b], p.j, pose_of(p.centre).asTPose(), anchor ? reloc.place_sigma_xy : lopt.sigma_xy, anchor ? place_yaw : lopt.sigma_yaw_deg, pr);
    if (pr.accepted) std::copy(pr.Z, pr.Z + 12, Z);
    rep.pairs.push_back(pr);
    return pr.accepted;
  };
  const JoinCandidates cand = join_candidates(pv.mapFrames(), fb, jopt, top_k, reloc.place_sectors, lopt, verify);
  for (const auto& kv : pv.report().seconds) rep.seconds[kv.first] += kv.second;
  for (const auto& kv : pv.report().counts) rep.counts[kv.first] += kv.second;
  rep.links_accepted = (uint32_t)cand.links.size();
  out.is_joined = rep.joined = rep.links_accepted >= jopt.min_links;
  if (!out.is_joined) return out;

  // ---- 5. B's poses in A's frame
  std::vector<double> poses(12 * (KA + KB));
  for (size_t k = 0; k < KA; k++) std::copy(A.frames[k].pose, A.frames[k].pose + 12, &poses[12 * k]);
  for (size_t b = 0; b < KB; b++) std::copy(B.frames[b].pose, B.frames[b].pose + 12, &poses[12 * (KA + b)]);
  std::vector<PoseGraphEdge> edges;
  for (const JoinLink& l : cand.links) {
    PoseGraphEdge e;
    e.a = l.j; e.b = (uint32_t)(KA + l.b);
    std::copy(l.Z, l.Z + 12, e.Z);
    edges.push_back(e);
  }
  PoseGraphResult g;
  {
    Timer t(rep, "optimize");
    g = optimize_pose_graph_anchored(poses, KA, {}, edges, lopt);
  }
  rep.cost_before = g.cost_before;
  rep.cost_after = g.cost_after;
  rep.optimizer_iterations = g.iterations;

  // ---- 6. A's frames, then B's with the new poses
  out.joined.frames.reserve(KA + KB);
  for (size_t b = 0; b < KB; b++) {
    out.joined.frames.push_back(B.frames[b]);
    std::copy(&g.poses[12 * (KA + b)], &g.poses[12 * (KA + b)] + 12, out.joined.frames.back().pose);
  }
  return out;
}

SessionJoinReport join_sessions_file(const std::string& keyframe_file_a, const std::string& keyframe_file_b, const Config& pipeline,
                                     const std::string& output_keyframe_file, std::shared_ptr<DeviceContext> ctx) {
  const SessionJoinResult r =
      join_sessions(molahip_host::read_keyframe_file(keyframe_file_a), molahip_host::read_keyframe_file(keyframe_file_b), pipeline, std::move(ctx));
  if (r.is_joined) molahip_host::write_keyframe_file(output_keyframe_file, r.joined);
  return r.report;
}

}  // namespace mola_hip
