// loop_closure.cpp -- see mola_lidar_odometry_hip/LoopClosure.h.  Host logic only: every point touches the GPU through the calls
// the relocalization already makes (mh_place_*, mh_map_insert_frames, mh_score_poses, the ICP of mp2p_icp_hip).
#include "mola_lidar_odometry_hip/LoopClosure.h"
#include "mola_lidar_odometry_hip/SessionJoin.h"
#include "loop_closure_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace mola_hip {

using namespace mp2p_icp_hip;

namespace {

constexpr double kDeg2Rad = M_PI / 180.0;

struct Stage {  // adds the wall time of its scope to a report entry, and one to its call count
  std::map<std::string, double>& sec;
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  Stage(LoopReport& r, const char* n, bool count = true) : sec(r.seconds), name(n) { if (count) r.counts[n] += 1.0; }
  ~Stage() { sec[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

CPose3D pose_of(const double* T) {
  CPose3D p;
  std::copy(T, T + 12, p.T);
  return p;
}

}  // namespace

// ================================================================== options
LoopClosureOptions LoopClosureOptions::FromConfig(const Config& cfg) {
  LoopClosureOptions o;
  o.sigma = LidarOdometry::Params().initial_sigma;
  if (cfg.has("params") && cfg["params"].has("adaptive_threshold") && cfg["params"]["adaptive_threshold"].has("initial_sigma"))
    o.sigma = strtod(cfg["params"]["adaptive_threshold"]["initial_sigma"].asString().c_str(), nullptr);
  if (cfg.has("loop_closure") && !cfg["loop_closure"].isNull()) {
    const Config& c = cfg["loop_closure"];
    auto num = [&](const char* k, double& v) {
      if (c.has(k) && !c[k].isNull()) v = strtod(c[k].asString().c_str(), nullptr);
    };
    auto cnt = [&](const char* k, uint32_t& v, double least) {
      if (!c.has(k) || c[k].isNull()) return;
      const double d = strtod(c[k].asString().c_str(), nullptr);
      if (!(d >= least) || !(d <= 4294967295.0))
        throw std::runtime_error(std::string("loop_closure: ") + k + " must be an integer >= " + std::to_string((int)least));
      v = (uint32_t)d;
    };
    num("min_travel", o.min_travel);
    num("gate_base", o.gate_base);
    num("gate_rate", o.gate_rate);
    cnt("max_place_dist", o.max_place_dist, 0.0);
    cnt("top_k", o.top_k, 1.0);
    num("min_travel_between_closures", o.min_travel_between_closures);
    num("submap_radius", o.submap_radius);
    num("sigma_xy", o.sigma_xy);
    num("sigma_yaw_deg", o.sigma_yaw_deg);
    num("sigma", o.sigma);
    num("min_quality", o.min_quality);
    num("odometry_sigma_xyz", o.odometry_sigma_xyz);
    num("odometry_sigma_rot_deg", o.odometry_sigma_rot_deg);
    num("loop_sigma_xyz", o.loop_sigma_xyz);
    num("loop_sigma_rot_deg", o.loop_sigma_rot_deg);
    cnt("max_iterations", o.max_iterations, 0.0);
    num("min_step", o.min_step);
  }
  o.validate();
  return o;
}

void LoopClosureOptions::validate() const {
  auto positive = [](const char* k, double v) {
    if (!(v > 0.0) || !std::isfinite(v)) throw std::runtime_error(std::string("loop_closure: ") + k + " must be finite and > 0");
  };
  auto not_negative = [](const char* k, double v) {
    if (!(v >= 0.0) || !std::isfinite(v)) throw std::runtime_error(std::string("loop_closure: ") + k + " must be finite and >= 0");
  };
  not_negative("min_travel", min_travel);
  not_negative("gate_base", gate_base);
  not_negative("gate_rate", gate_rate);
  if (top_k < 1) throw std::runtime_error("loop_closure: top_k must be an integer >= 1");
  not_negative("min_travel_between_closures", min_travel_between_closures);
  not_negative("submap_radius", submap_radius);
  positive("sigma_xy", sigma_xy);
  positive("sigma_yaw_deg", sigma_yaw_deg);
  positive("sigma", sigma);
  not_negative("min_quality", min_quality);
  positive("odometry_sigma_xyz", odometry_sigma_xyz);
  positive("odometry_sigma_rot_deg", odometry_sigma_rot_deg);
  positive("loop_sigma_xyz", loop_sigma_xyz);
  positive("loop_sigma_rot_deg", loop_sigma_rot_deg);
  not_negative("min_step", min_step);
}

OnlineLoopClosureOptions OnlineLoopClosureOptions::FromConfig(const Config& cfg) {
  OnlineLoopClosureOptions o;
  if (cfg.has("online_loop_closure") && !cfg["online_loop_closure"].isNull()) {
    const Config& c = cfg["online_loop_closure"];
    auto flag = [&](const char* k, bool& v) {
      if (!c.has(k) || c[k].isNull()) return;
      const std::string s = c[k].asString();
      if (s == "true" || s == "True" || s == "1" || s == "yes") v = true;
      else if (s == "false" || s == "False" || s == "0" || s == "no") v = false;
      else throw std::runtime_error(std::string("online_loop_closure: ") + k + " must be true or false");
    };
    flag("enabled", o.enabled);
    flag("correct_driver", o.correct_driver);
    if (c.has("check_every_n_keyframes") && !c["check_every_n_keyframes"].isNull()) {
      const double d = strtod(c["check_every_n_keyframes"].asString().c_str(), nullptr);
      if (!(d >= 1.0) || !(d <= 4294967295.0) || d != std::floor(d))
        throw std::runtime_error("online_loop_closure: check_every_n_keyframes must be an integer >= 1");
      o.check_every_n_keyframes = (uint32_t)d;
    }
  }
  o.validate();
  return o;
}

void OnlineLoopClosureOptions::validate() const {
  if (check_every_n_keyframes < 1) throw std::runtime_error("online_loop_closure: check_every_n_keyframes must be an integer >= 1");
}

// ================================================================== candidate selection
namespace {
double path_step(const double* a, const double* b) {  // |t_b - t_a|
  const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
  return std::sqrt(dx * dx + dy * dy + dz * dz);
}
}  // namespace

std::vector<double> path_lengths(const std::vector<LoopFrame>& frames) {
  std::vector<double> s(frames.size(), 0.0);
  for (size_t k = 1; k < frames.size(); k++) s[k] = s[k - 1] + path_step(frames[k - 1].pose, frames[k].pose);
  return s;
}

bool loop_candidates_step(const std::vector<LoopFrame>& frames, const std::vector<double>& s, size_t i, const LoopClosureOptions& opt,
                          LoopCandidateState& state, const std::function<bool(const LoopPair&)>& verify, std::vector<LoopPair>& tried) {
  if (!frames[i].has_points) return false;
  if (state.closed && s[i] < state.s_closed + opt.min_travel_between_closures) return false;
  uint32_t n = 0;
  for (const PlaceIndex::Match& m : frames[i].matches) {
    if (n >= opt.top_k) break;
    const size_t j = m.frame;
    if (j >= i || !frames[j].has_points) continue;
    const double travel = s[i] - s[j];
    if (!(travel >= opt.min_travel)) continue;
    if (!(path_step(frames[j].pose, frames[i].pose) <= opt.gate_base + opt.gate_rate * travel)) continue;
    if (opt.max_place_dist != 0 && m.dist > opt.max_place_dist) continue;
    n++;
    LoopPair p;
    p.i = (uint32_t)i; p.j = (uint32_t)j; p.shift = m.shift; p.dist = m.dist;
    tried.push_back(p);
    if (!verify || verify(p)) {
      state.closed = true;
      state.s_closed = s[i];
      return true;
    }
  }
  return false;
}

std::vector<LoopPair> loop_candidates(const std::vector<LoopFrame>& frames, const LoopClosureOptions& opt,
                                      const std::function<bool(const LoopPair&)>& verify) {
  const std::vector<double> s = path_lengths(frames);
  std::vector<LoopPair> tried;
  LoopCandidateState state;
  for (size_t i = 0; i < frames.size(); i++) (void)loop_candidates_step(frames, s, i, opt, state, verify, tried);
  return tried;
}

// ================================================================== pose graph
namespace {

struct GraphEdge {
  uint32_t a, b;
  CPose3D Z;
  double w[6];
};

// r = [t(E); log R(E)], E = Z^-1 T_a^-1 T_b; optionally the Jacobians (6x6 row-major) to the right perturbations [dt; dtheta] of a and b
void edge_residual(const GraphEdge& e, const CPose3D& Ta, const CPose3D& Tb, double r[6], double* Ja, double* Jb) {
  const CPose3D M = Tb - Ta;   // T_a^-1 T_b
  const CPose3D E = M - e.Z;   // Z^-1 M
  r[0] = E.T[3]; r[1] = E.T[7]; r[2] = E.T[11];
  E.so3Log(r + 3);
  if (!Ja) return;
  const double *p = r + 3;
  const double th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2], th = std::sqrt(th2);
  const double c = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + std::cos(th)) / (2.0 * th * std::sin(th));
  const double P[9] = {0, -p[2], p[1], p[2], 0, -p[0], -p[1], p[0], 0};
  double Jri[9];  // I + P / 2 + c P^2
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double pp = 0;
      for (int k = 0; k < 3; k++) pp += P[i * 3 + k] * P[k * 3 + j];
      Jri[i * 3 + j] = (i == j ? 1.0 : 0.0) + 0.5 * P[i * 3 + j] + c * pp;
    }
  std::fill(Ja, Ja + 36, 0.0);
  std::fill(Jb, Jb + 36, 0.0);
  const double tm[3] = {M.T[3], M.T[7], M.T[11]};
  const double TMx[9] = {0, -tm[2], tm[1], tm[2], 0, -tm[0], -tm[1], tm[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Jb[i * 6 + j] = E.T[i * 4 + j];                  // dt / dt_b = R_E
      Jb[(3 + i) * 6 + 3 + j] = Jri[i * 3 + j];        // dtheta / dtheta_b = Jr^-1
      Ja[i * 6 + j] = -e.Z.T[j * 4 + i];               // dt / dt_a = -R_Z^T
      double v = 0, u = 0;
      for (int k = 0; k < 3; k++) {
        v += e.Z.T[k * 4 + i] * TMx[k * 3 + j];        // dt / dtheta_a = R_Z^T [t_M]x
        u -= Jri[i * 3 + k] * M.T[j * 4 + k];          // dtheta / dtheta_a = -Jr^-1 R_M^T
      }
      Ja[i * 6 + 3 + j] = v;
      Ja[(3 + i) * 6 + 3 + j] = u;
    }
}

double graph_cost(const std::vector<GraphEdge>& edges, const std::vector<CPose3D>& T) {
  double cost = 0;
  for (const GraphEdge& e : edges) {
    double r[6];
    edge_residual(e, T[e.a], T[e.b], r, nullptr, nullptr);
    for (int k = 0; k < 6; k++) cost += e.w[k] * r[k] * r[k];
  }
  return cost;
}

// symmetric positive definite matrix in lower profile storage: row r holds columns first[r] .. r
struct Profile {
  std::vector<size_t> first, off;
  std::vector<double> v;
  double& at(size_t r, size_t c) { return v[off[r] + (c - first[r])]; }
  double get(size_t r, size_t c) const { return v[off[r] + (c - first[r])]; }
  // in place L L^T; false when a pivot is not positive
  bool factor() {
    const size_t n = first.size();
    for (size_t i = 0; i < n; i++) {
      for (size_t j = first[i]; j <= i; j++) {
        double sum = get(i, j);
        const size_t k0 = std::max(first[i], first[j]);
        const double *li = &v[off[i] + (k0 - first[i])], *lj = &v[off[j] + (k0 - first[j])];
        for (size_t k = k0; k < j; k++) sum -= *li++ * *lj++;
        if (j < i) {
          at(i, j) = sum / get(j, j);
        } else {
          if (!(sum > 0.0) || !std::isfinite(sum)) return false;
          at(i, i) = std::sqrt(sum);
        }
      }
    }
    return true;
  }
  void solve(std::vector<double>& x) const {  // x: right-hand side in, solution out
    const size_t n = first.size();
    for (size_t i = 0; i < n; i++) {
      double sum = x[i];
      for (size_t k = first[i]; k < i; k++) sum -= get(i, k) * x[k];
      x[i] = sum / get(i, i);
    }
    for (size_t i = n; i-- > 0;) {
      x[i] /= get(i, i);
      for (size_t k = first[i]; k < i; k++) x[k] -= get(i, k) * x[i];
    }
  }
};

void edge_weights(double sxyz, double srot_deg, double w[6]) {
  const double srot = srot_deg * kDeg2Rad;
  for (int k = 0; k < 3; k++) w[k] = 1.0 / (sxyz * sxyz), w[3 + k] = 1.0 / (srot * srot);
}

// The Levenberg-Marquardt loop of LoopClosure.h over the nodes T: the first n_fixed stay as they are, node v >= n_fixed is variable
// block v - n_fixed.  Fills out's costs and iteration count; T holds the optimum.
void solve_graph(std::vector<CPose3D>& T, const size_t n_fixed, const std::vector<GraphEdge>& edges, const LoopClosureOptions& opt, PoseGraphResult& out) {
  const size_t K = T.size();
  // the envelope: a block row starts at the lowest block it shares an edge with
  const size_t nb = K - n_fixed, n = 6 * nb;
  std::vector<size_t> first_block(nb);
  for (size_t v = 0; v < nb; v++) first_block[v] = v;
  for (const GraphEdge& e : edges) {
    if (e.a < n_fixed || e.b < n_fixed) continue;
    const size_t lo = std::min(e.a, e.b) - n_fixed, hi = std::max(e.a, e.b) - n_fixed;
    first_block[hi] = std::min(first_block[hi], lo);
  }
  Profile H;
  H.first.resize(n);
  H.off.resize(n);
  size_t total = 0;
  for (size_t r = 0; r < n; r++) {
    H.first[r] = 6 * first_block[r / 6];
    H.off[r] = total;
    total += r - H.first[r] + 1;
  }
  std::vector<double> Hv(total), g(n), delta(n);
  std::vector<CPose3D> Tn(T);
  double cost = graph_cost(edges, T);
  out.cost_before = cost;
  out.costs.push_back(cost);
  double lambda = 0.0;
  for (uint32_t it = 0; it < opt.max_iterations; it++) {
    // ---- normal equations at T
    H.v.assign(total, 0.0);
    std::fill(g.begin(), g.end(), 0.0);
    for (const GraphEdge& e : edges) {
      double r[6], J[2][36];
      edge_residual(e, T[e.a], T[e.b], r, J[0], J[1]);
      const uint32_t node[2] = {e.a, e.b};
      for (int p = 0; p < 2; p++) {
        if (node[p] < n_fixed) continue;
        const size_t rp = 6 * (node[p] - n_fixed);
        for (int i = 0; i < 6; i++) {
          double s = 0;
          for (int k = 0; k < 6; k++) s += J[p][k * 6 + i] * e.w[k] * r[k];
          g[rp + i] += s;
        }
        for (int q = 0; q < 2; q++) {
          if (node[q] < n_fixed || node[q] > node[p]) continue;  // lower triangle: block row p, block column q <= p
          const size_t cq = 6 * (node[q] - n_fixed);
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
              if (p == q && j > i) continue;
              double s = 0;
              for (int k = 0; k < 6; k++) s += J[p][k * 6 + i] * e.w[k] * J[q][k * 6 + j];
              H.at(rp + i, cq + j) += s;
            }
        }
      }
    }
    Hv = H.v;
    // ---- a step that does not raise the cost: undamped first, damped after a refusal
    bool accepted = false;
    double maxd = 0.0;
    for (int attempt = 0; attempt < 12; attempt++) {
      H.v = Hv;
      if (lambda > 0.0)
        for (size_t r = 0; r < n; r++) H.at(r, r) *= 1.0 + lambda;
      if (!H.factor()) {
        lambda = std::max(10.0 * lambda, 1e-6);
        continue;
      }
      for (size_t r = 0; r < n; r++) delta[r] = -g[r];
      H.solve(delta);
      maxd = 0.0;
      for (double d : delta) maxd = std::max(maxd, std::fabs(d));
      if (!std::isfinite(maxd)) {
        lambda = std::max(10.0 * lambda, 1e-6);
        continue;
      }
      for (size_t v = 0; v < n_fixed; v++) Tn[v] = T[v];
      for (size_t v = 0; v < nb; v++) Tn[v + n_fixed] = T[v + n_fixed] + CPose3D::FromRotVecAndTranslation(&delta[6 * v + 3], &delta[6 * v]);
      const double cn = graph_cost(edges, Tn);
      if (cn <= cost) {
        T.swap(Tn);
        cost = cn;
        out.costs.push_back(cost);
        lambda = lambda > 1e-9 ? 0.1 * lambda : 0.0;
        accepted = true;
        break;
      }
      if (maxd < opt.min_step) break;  // converged: what is left is below the cost's rounding
      lambda = std::max(10.0 * lambda, 1e-6);
    }
    out.iterations++;
    if (!accepted || maxd < opt.min_step) break;
  }
  out.cost_after = cost;
}

}  // namespace

PoseGraphResult optimize_pose_graph(const std::vector<double>& poses, const std::vector<PoseGraphEdge>& loops, const LoopClosureOptions& opt) {
  if (poses.size() % 12) throw std::runtime_error("optimize_pose_graph: 12 values per pose");
  const size_t K = poses.size() / 12;
  for (const PoseGraphEdge& e : loops) {
    if (e.a >= K || e.b >= K)
      throw std::runtime_error("optimize_pose_graph: a loop edge names node " + std::to_string(std::max(e.a, e.b)) + " of " + std::to_string(K));
    if (e.a == e.b) throw std::runtime_error("optimize_pose_graph: a loop edge from node " + std::to_string(e.a) + " to itself");
  }
  for (double v : poses)
    if (!std::isfinite(v)) throw std::runtime_error("optimize_pose_graph: non-finite pose");
  PoseGraphResult out;
  out.poses = poses;
  if (loops.empty() || K < 2) {  // the chain's residuals are zero by construction
    out.costs.push_back(0.0);
    return out;
  }
  std::vector<CPose3D> T(K);
  for (size_t k = 0; k < K; k++) T[k] = pose_of(&poses[12 * k]);
  std::vector<GraphEdge> edges;
  edges.reserve(K - 1 + loops.size());
  for (size_t k = 1; k < K; k++) {
    GraphEdge e;
    e.a = (uint32_t)(k - 1); e.b = (uint32_t)k;
    e.Z = T[k] - T[k - 1];
    edge_weights(opt.odometry_sigma_xyz, opt.odometry_sigma_rot_deg, e.w);
    edges.push_back(e);
  }
  for (const PoseGraphEdge& l : loops) {
    GraphEdge e;
    e.a = l.a; e.b = l.b;
    e.Z = pose_of(l.Z);
    edge_weights(opt.loop_sigma_xyz, opt.loop_sigma_rot_deg, e.w);
    edges.push_back(e);
  }
  solve_graph(T, 1, edges, opt, out);  // node 0 is fixed
  for (size_t k = 1; k < K; k++) std::copy(T[k].T, T[k].T + 12, &out.poses[12 * k]);
  return out;
}

// (SessionJoin.h; here because it runs on solve_graph)
PoseGraphResult optimize_pose_graph_anchored(const std::vector<double>& poses, size_t n_fixed, const std::vector<uint32_t>& chain_starts,
                                             const std::vector<PoseGraphEdge>& links, const LoopClosureOptions& opt) {
  const char* who = "optimize_pose_graph_anchored: ";
  if (poses.size() % 12) throw std::runtime_error(std::string(who) + "12 values per pose");
  const size_t K = poses.size() / 12;
  if (n_fixed < 1 || n_fixed > K) throw std::runtime_error(std::string(who) + std::to_string(n_fixed) + " fixed nodes of " + std::to_string(K) + ": at least one, at most all");
  for (double v : poses)
    if (!std::isfinite(v)) throw std::runtime_error(std::string(who) + "non-finite pose");
  // chain[k]: the first node of free node k's chain
  std::vector<bool> starts(K, false);
  if (n_fixed < K) starts[n_fixed] = true;
  for (uint32_t c : chain_starts) {
    if (c < n_fixed || c >= K) throw std::runtime_error(std::string(who) + "a chain cannot start at node " + std::to_string(c) + " (" + std::to_string(n_fixed) + " fixed, " + std::to_string(K) + " in all)");
    starts[c] = true;
  }
  std::vector<size_t> chain(K, 0);
  for (size_t k = n_fixed; k < K; k++) chain[k] = starts[k] ? k : chain[k - 1];
  for (const PoseGraphEdge& e : links) {
    if (e.a >= K || e.b >= K) throw std::runtime_error(std::string(who) + "an edge names node " + std::to_string(std::max(e.a, e.b)) + " of " + std::to_string(K));
    if (e.a == e.b) throw std::runtime_error(std::string(who) + "an edge from node " + std::to_string(e.a) + " to itself");
    if (e.a < n_fixed && e.b < n_fixed)
      throw std::runtime_error(std::string(who) + "the edge (" + std::to_string(e.a) + ", " + std::to_string(e.b) + ") joins two fixed nodes");
  }
  opt.validate();
  PoseGraphResult out;
  out.poses = poses;
  std::vector<CPose3D> T(K);
  for (size_t k = 0; k < K; k++) T[k] = pose_of(&poses[12 * k]);
  // ---- the chain edges, from the poses as given (a rigid placement does not change them)
  std::vector<GraphEdge> edges;
  for (size_t k = n_fixed + 1; k < K; k++) {
    if (starts[k]) continue;
    GraphEdge e;
    e.a = (uint32_t)(k - 1); e.b = (uint32_t)k;
    e.Z = T[k] - T[k - 1];
    edge_weights(opt.odometry_sigma_xyz, opt.odometry_sigma_rot_deg, e.w);
    edges.push_back(e);
  }
  // ---- every chain placed by its first edge from a fixed node
  std::vector<size_t> n_edges(K, 0);  // per chain (indexed by its first node)
  std::vector<bool> placed(K, false);
  bool overdetermined = false;
  for (const PoseGraphEdge& l : links) {
    const bool a_fixed = l.a < n_fixed, b_fixed = l.b < n_fixed;
    if (!a_fixed) n_edges[chain[l.a]]++;
    if (!b_fixed && (a_fixed || chain[l.b] != chain[l.a])) n_edges[chain[l.b]]++;
    if (!a_fixed && !b_fixed) overdetermined = true;
    if (a_fixed == b_fixed) continue;
    const size_t c = chain[a_fixed ? l.b : l.a];
    if (placed[c]) continue;
    placed[c] = true;
    const CPose3D Z = pose_of(l.Z), I;
    const CPose3D G = a_fixed ? (T[l.a] + Z) + (I - T[l.b]) : (T[l.b] + (I - Z)) + (I - T[l.a]);
    for (size_t k = c; k < K && chain[k] == c; k++) T[k] = G + T[k];
  }
  for (size_t k = n_fixed; k < K; k++) {
    if (!starts[k]) continue;
    if (!placed[k])
      throw std::runtime_error(std::string(who) + "the chain that starts at node " + std::to_string(k) + " has no edge from a fixed node: its frame is undetermined");
    if (n_edges[k] > 1) overdetermined = true;
  }
  for (size_t k = n_fixed; k < K; k++) std::copy(T[k].T, T[k].T + 12, &out.poses[12 * k]);
  if (!overdetermined) {  // every residual is zero by construction
    out.costs.push_back(0.0);
    return out;
  }
  for (const PoseGraphEdge& l : links) {
    GraphEdge e;
    e.a = l.a; e.b = l.b;
    e.Z = pose_of(l.Z);
    edge_weights(opt.loop_sigma_xyz, opt.loop_sigma_rot_deg, e.w);
    edges.push_back(e);
  }
  solve_graph(T, n_fixed, edges, opt, out);
  for (size_t k = n_fixed; k < K; k++) std::copy(T[k].T, T[k].T + 12, &out.poses[12 * k]);
  return out;
}

// ================================================================== report
std::string LoopReport::toJson() const {
  std::string o = "{\"pairs\": [";
  char buf[64];
  auto num = [&](double v) {
    snprintf(buf, sizeof(buf), "%.17g", v);
    return std::string(std::isfinite(v) ? buf : "null");
  };
  for (size_t k = 0; k < pairs.size(); k++) {
    const Pair& p = pairs[k];
    o += std::string(k ? ", " : "") + "{\"i\": " + std::to_string(p.i) + ", \"j\": " + std::to_string(p.j) + ", \"shift\": " + std::to_string(p.shift) +
         ", \"dist\": " + std::to_string(p.dist) + ", \"candidates\": " + std::to_string(p.candidates) + ", \"ranks\": [";
    for (size_t c = 0; c < p.ranks.size(); c++) o += (c ? ", " : "") + std::to_string(p.ranks[c]);
    o += "], \"quality\": " + num(p.quality) + ", \"iterations\": " + std::to_string(p.iterations) + ", \"accepted\": " + (p.accepted ? "true" : "false") +
         ", \"Z\": [";
    for (int c = 0; c < 12; c++) o += (c ? ", " : "") + num(p.Z[c]);
    o += "]}";
  }
  o += "], \"cost_before\": " + num(cost_before) + ", \"cost_after\": " + num(cost_after) + ", \"optimizer_iterations\": " + std::to_string(optimizer_iterations);
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

// ================================================================== what close_loops and OnlineLoopCloser share
namespace {

struct IcpLayers {
  std::map<std::string, int> local_layers;  // local layer name -> the target map whose stored points it holds
  std::string gname, lname;                 // the (global, local) layers candidates are scored on
};

IcpLayers icp_layers(ICP& icp, const std::vector<std::string>& map_names, const std::string& who) {
  auto map_index_of = [&](const std::string& name) -> int {
    for (size_t k = 0; k < map_names.size(); k++)
      if (map_names[k] == name) return (int)k;
    return -1;
  };
  IcpLayers out;
  for (const auto& m : icp.matchers()) {
    if (!m->enabled) continue;
    const std::vector<Matcher_Points_DistanceThreshold::LayerMatch>* lm = nullptr;
    auto* pm = dynamic_cast<Matcher_Points_DistanceThreshold*>(m.get());
    if (pm) lm = &pm->pointLayerMatches;
    else if (auto* pl = dynamic_cast<Matcher_Point2Plane*>(m.get())) lm = &pl->pointLayerMatches;
    if (!lm) continue;
    for (const auto& e : *lm) {
      const int k = map_index_of(e.global);
      if (k < 0)
        throw std::runtime_error(who + ": the ICP block matches against the global layer '" + e.global +
                                 "', which is no target map of the key-frame file's header");
      const auto it = out.local_layers.find(e.local);
      if (it != out.local_layers.end() && it->second != k)
        throw std::runtime_error(who + ": the local layer '" + e.local + "' is matched against two target maps; a key-frame stores one input layer per map");
      out.local_layers[e.local] = k;
    }
    if (pm && out.gname.empty() && !pm->pointLayerMatches.empty()) {
      out.gname = pm->pointLayerMatches[0].global;
      out.lname = pm->pointLayerMatches[0].local;
    }
  }
  if (out.gname.empty()) throw std::runtime_error(who + ": the ICP block has no enabled Matcher_Points_DistanceThreshold to score candidates with");
  return out;
}

void refuse_unbuildable_targets(const std::vector<molahip_host::KeyFrameTarget>& maps, const std::string& who) {
  for (const auto& t : maps) {
    if (t.class_name == "CVoxelMap")
      throw std::runtime_error(who + ": target map '" + t.name + "' is a '" + t.class_name + "': an occupancy map cannot be built from "
                               "key-frames, so no submap to verify a loop in (HashedVoxelPointCloud, NDT and SparseTreesPointCloud can)");
    if (!molahip_host::local_map_class_known(t.class_name))
      throw std::runtime_error(who + ": target map '" + t.name + "' is of the unknown class '" + t.class_name + "'");
  }
}

bool usable(const molahip_host::KeyFrame& f) { return f.has_points && !f.layers.empty() && !f.layers[0].x.empty(); }

}  // namespace

void check_loop_closure_icp(ICP& icp, const std::vector<std::string>& map_names, const std::string& who) { (void)icp_layers(icp, map_names, who); }

// The ICP the driver relocalizes with (its variables as after reset()), the place database, the frames' selection data, the loop
// edges and the report: close_loops fills `frames` and `s` for the whole set before it selects, OnlineLoopCloser frame by frame.
struct LoopCloserCore {
  const LoopClosureOptions opt;
  const LidarOdometry::RelocalizationOptions reloc;
  const std::vector<molahip_host::KeyFrameTarget> maps;
  std::shared_ptr<DeviceContext> ctx;
  ICP::Ptr icp;
  Parameters icp_params;
  ParameterSource source;
  IcpLayers layers;
  double min_range = 0, thr = 0;
  mh_place_params pp{};
  mh_place_db* db = nullptr;
  size_t dsize = 0;
  std::vector<uint32_t> frame_of;                          // database entry -> frame
  const std::vector<molahip_host::KeyFrame>* kf = nullptr;  // the frames by index: their layers
  std::vector<LoopFrame> frames;                           // ... their recorded (raw) poses and match lists
  std::vector<double> s;                                   // ... and path lengths
  std::vector<PoseGraphEdge> loops;
  LoopReport rep;

  LoopCloserCore(const std::vector<molahip_host::KeyFrameTarget>& maps_, const Config& pipeline, std::shared_ptr<DeviceContext> ctx_, const std::string& who)
      : opt(LoopClosureOptions::FromConfig(pipeline)), reloc(relocalization_options(pipeline)), maps(maps_), ctx(std::move(ctx_)) {
    refuse_unbuildable_targets(maps, who);
    const Config& block = pipeline.has("icp_settings_without_vel") ? pipeline["icp_settings_without_vel"] : pipeline["icp_settings_with_vel"];
    if (!ctx) ctx = DeviceContext::Default();
    auto made = icp_pipeline_from_yaml(block, ctx);
    icp = std::get<0>(made);
    icp_params = std::get<1>(made);
    icp->attachToParameterSource(source);
    icp->setKeepFinalPairings(false);
    icp->fuseGatedMatchers(true);
    icp->fuseMultiPairings(true);
    icp->fusePlaneMatchers(true);
    std::vector<std::string> names;
    for (const auto& t : maps) names.push_back(t.name);
    layers = icp_layers(*icp, names, who);
    min_range = LidarOdometry::Params().absolute_minimum_sensor_range;
    if (pipeline.has("params") && pipeline["params"].has("absolute_minimum_sensor_range"))
      min_range = strtod(pipeline["params"]["absolute_minimum_sensor_range"].asString().c_str(), nullptr);
    for (const char* v : {"vx", "vy", "vz", "wx", "wy", "wz", "robot_x", "robot_y", "robot_z", "robot_yaw", "robot_pitch", "robot_roll", "ICP_ITERATION",
                          "icp_iterations", "SENSOR_TIME_OFFSET", "twistCorrectionCount"})
      source.updateVariable(v, 0.0);
    source.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", opt.sigma);
    source.updateVariable("INSTANTANEOUS_SENSOR_MAX_RANGE", 20.0);
    source.updateVariable("ESTIMATED_SENSOR_MAX_RANGE", min_range);
    pp.n_rings = reloc.place_rings; pp.n_sectors = reloc.place_sectors;
    pp.min_range = (float)reloc.place_min_range; pp.max_range = (float)reloc.place_max_range;
    pp.z_min = (float)reloc.place_z_min; pp.z_max = (float)reloc.place_z_max;
    check(mh_place_db_create(ctx->get(), &pp, &db), "mh_place_db_create");
    dsize = (size_t)pp.n_rings * pp.n_sectors;
    for (size_t k = 0; k < maps.size(); k++)
      if (maps[k].name == layers.gname) thr = 0.5 * (double)maps[k].params.voxel_size;
  }
  ~LoopCloserCore() { if (db) (void)mh_place_db_destroy(db); }
  LoopCloserCore(const LoopCloserCore&) = delete;
  LoopCloserCore& operator=(const LoopCloserCore&) = delete;

  // the descriptor of a frame's first stored layer (counted as one "describe")
  std::vector<uint8_t> describe(const molahip_host::KeyFrame& f) {
    Stage st(rep, "describe");
    const auto& l = f.layers[0];
    DevicePointCloud layer(ctx);
    layer.setPoints(l.x.data(), l.y.data(), l.z.data(), l.x.size());
    std::vector<uint8_t> d(dsize);
    check(mh_place_describe(layer.handle(), &pp, d.data(), MH_MEM_HOST), "mh_place_describe");
    return d;
  }
  // ... appended to the database as frame k's (its time goes to "describe")
  void add(const std::vector<uint8_t>& d, size_t k) {
    Stage st(rep, "describe", false);
    check(mh_place_db_add(db, d.data(), 1, MH_MEM_HOST), "mh_place_db_add");
    frame_of.push_back((uint32_t)k);
  }
  // every descriptor of the database against `d`, ranked by (dist ascending, frame ascending)
  std::vector<PlaceIndex::Match> search(const std::vector<uint8_t>& d) {
    Stage st(rep, "search");
    std::vector<PlaceIndex::Match> m;
    if (frame_of.empty()) return m;  // (an empty database has nothing to launch on)
    std::vector<mh_place_match> found(frame_of.size());
    check(mh_place_search(db, d.data(), MH_MEM_HOST, found.data(), MH_MEM_HOST), "mh_place_search");
    m.resize(found.size());
    for (size_t k = 0; k < found.size(); k++) m[k] = PlaceIndex::Match{frame_of[k], found[k].shift, found[k].dist};
    std::stable_sort(m.begin(), m.end(), [](const PlaceIndex::Match& a, const PlaceIndex::Match& b) { return a.dist != b.dist ? a.dist < b.dist : a.frame < b.frame; });
    return m;
  }

  // verification of one pair on the device; an accepted one becomes a loop edge
  bool verify(const LoopPair& c) {
    LoopReport::Pair pr;
    pr.i = c.i; pr.j = c.j; pr.shift = c.shift; pr.dist = c.dist;
    const CPose3D Ti = pose_of(frames[c.i].pose), Tj = pose_of(frames[c.j].pose);
    verify_at((*kf)[c.i], c.j, [&](size_t q) { return s[c.i] - s[q] >= opt.min_travel; }, (Ti - Tj).asTPose(), opt.sigma_xy, opt.sigma_yaw_deg, pr);
    if (pr.accepted) {
      PoseGraphEdge e;
      e.a = c.j; e.b = c.i;
      std::copy(pr.Z, pr.Z + 12, e.Z);
      loops.push_back(e);
    }
    rep.pairs.push_back(pr);
    return pr.accepted;
  }

  // The verification itself: `observed` (a frame with points, of this set or of another) against the submap around frame j -- the
  // frames q with points, |s_q - s_j| <= submap_radius and keep(q), at T_j^-1 T_q -- from the grid of (sigma_xy, sigma_yaw_deg)
  // around `centre`, the guess of the observed frame in frame j.  Fills pr's candidates, ranks, quality, iterations, Z and accepted.
  void verify_at(const molahip_host::KeyFrame& observed, size_t j, const std::function<bool(size_t)>& keep, const TPose3D& centre, double sigma_xy,
                 double sigma_yaw_deg, LoopReport::Pair& pr) {
    const std::vector<molahip_host::KeyFrame>& set_frames = *kf;
    const size_t K = frames.size();
    const CPose3D Tj = pose_of(frames[j].pose);
    metric_map_t glob, obs;
    {
      Stage st(rep, "submap");
      for (size_t k = 0; k < maps.size(); k++) {
        const auto& t = maps[k];
        molahip_host::LocalMapRecord empty;
        empty.name = t.name;
        empty.class_name = t.class_name;
        empty.params = t.params;
        auto map = make_local_map(empty, ctx);
        std::vector<PosedFrame> pf;
        for (size_t q = 0; q < K; q++) {
          if (!frames[q].has_points || !(std::fabs(s[q] - s[j]) <= opt.submap_radius) || !keep(q)) continue;
          for (const auto& l : set_frames[q].layers) {  // step order
            if (l.map_index != k) continue;
            PosedFrame f;
            f.x = l.x.data(); f.y = l.y.data(); f.z = l.z.data();
            f.n = l.x.size();
            f.pose = pose_of(frames[q].pose) - Tj;
            pf.push_back(f);
          }
        }
        map->insertFrames(pf, 0);
        glob.layers[t.name] = map;
      }
      for (const auto& [name, k] : layers.local_layers) {
        std::vector<float> x, y, z;
        for (const auto& l : observed.layers) {
          if ((int)l.map_index != k) continue;
          x.insert(x.end(), l.x.begin(), l.x.end());
          y.insert(y.end(), l.y.begin(), l.y.end());
          z.insert(z.end(), l.z.begin(), l.z.end());
        }
        auto cloud = std::make_shared<DevicePointCloud>(ctx);
        cloud->setPoints(x.data(), y.data(), z.data(), x.size());
        obs.layers[name] = cloud;
      }
      ctx->synchronize();  // (the stage's time is the build's, not its enqueue's)
    }
    // the variables of this frame
    double range = 0.0;
    {
      const auto& l = observed.layers[0];
      for (size_t p = 0; p < l.x.size(); p++) {
        const double x = l.x[p], y = l.y[p], z = l.z[p], r2 = x * x + y * y + z * z;
        if (std::isfinite(r2)) range = std::max(range, r2);
      }
      range = std::max(std::sqrt(range), min_range);
    }
    source.updateVariable("ESTIMATED_SENSOR_MAX_RANGE", range);
    source.realize();
    if (!reloc.score_threshold.empty()) {
      std::string e = reloc.score_threshold;
      if (e.size() > 4 && e.compare(0, 3, "$f{") == 0 && e.back() == '}') e = e.substr(3, e.size() - 4);
      thr = evaluate_expression(e, source.getVariableValues());
    }
    const double step = reloc.step_xy > 0 ? reloc.step_xy : thr;
    double cov[36] = {0};
    cov[0] = cov[7] = sigma_xy * sigma_xy;
    cov[21] = (sigma_yaw_deg * kDeg2Rad) * (sigma_yaw_deg * kDeg2Rad);
    const std::vector<TPose3D> cand = relocalization_grid(centre, cov, step, reloc.step_yaw_deg * kDeg2Rad, reloc.sigmas, reloc.max_candidates);
    pr.candidates = (uint32_t)cand.size();
    const RelocalizationRefinement rr =
        score_rank_refine(*icp, icp_params, obs, glob, layers.gname, layers.lname, cand, thr, reloc.refine_top_k, &rep.seconds);
    rep.counts["score"] += 1.0;
    rep.counts["refine"] += (double)rr.ranks.size();
    pr.ranks = rr.ranks;
    if (rr.have) {
      pr.quality = rr.best.quality;
      pr.iterations = (uint32_t)rr.best.nIterations;
      std::copy(rr.best.optimal_tf.mean.T, rr.best.optimal_tf.mean.T + 12, pr.Z);
      pr.accepted = rr.best.quality >= opt.min_quality;
    }
  }

  // one optimisation over all frames, from their recorded (raw) poses and every loop edge so far
  std::vector<double> optimize(bool count = true) {
    const size_t K = frames.size();
    std::vector<double> poses(12 * K);
    for (size_t k = 0; k < K; k++) std::copy(frames[k].pose, frames[k].pose + 12, &poses[12 * k]);
    PoseGraphResult g;
    {
      Stage st(rep, "optimize", count);
      g = optimize_pose_graph(poses, loops, opt);
    }
    rep.cost_before = g.cost_before;
    rep.cost_after = g.cost_after;
    rep.optimizer_iterations = g.iterations;
    return std::move(g.poses);
  }
};

// ================================================================== the verification lent to session_join.cpp
PairVerifier::PairVerifier(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, std::shared_ptr<DeviceContext> ctx,
                           const std::string& who)
    : core_(std::make_unique<LoopCloserCore>(maps, pipeline, std::move(ctx), who)) {}
PairVerifier::~PairVerifier() = default;
void PairVerifier::setMapFrames(const std::vector<molahip_host::KeyFrame>& frames) {
  LoopCloserCore& c = *core_;
  c.kf = &frames;
  c.frames.assign(frames.size(), LoopFrame());
  for (size_t k = 0; k < frames.size(); k++) {
    std::copy(frames[k].pose, frames[k].pose + 12, c.frames[k].pose);
    c.frames[k].has_points = mola_hip::usable(frames[k]);
  }
  c.s = path_lengths(c.frames);
}
const std::vector<LoopFrame>& PairVerifier::mapFrames() const { return core_->frames; }
void PairVerifier::verify(const molahip_host::KeyFrame& observed, size_t j, const TPose3D& centre, double sigma_xy, double sigma_yaw_deg,
                          LoopReport::Pair& pr) {
  core_->verify_at(observed, j, [](size_t) { return true; }, centre, sigma_xy, sigma_yaw_deg, pr);
}
const LoopClosureOptions& PairVerifier::options() const { return core_->opt; }
const LidarOdometry::RelocalizationOptions& PairVerifier::relocalization() const { return core_->reloc; }
const mh_place_params& PairVerifier::placeParams() const { return core_->pp; }
const std::shared_ptr<DeviceContext>& PairVerifier::context() const { return core_->ctx; }
LoopReport& PairVerifier::report() { return core_->rep; }
bool PairVerifier::usable(const molahip_host::KeyFrame& f) { return mola_hip::usable(f); }
void PairVerifier::checkWithoutDevice(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, const std::string& who) {
  (void)LoopClosureOptions::FromConfig(pipeline);
  (void)relocalization_options(pipeline);
  refuse_unbuildable_targets(maps, who);
}

// ================================================================== close_loops
LoopClosureResult close_loops(const molahip_host::KeyFrameSet& set, const Config& pipeline, std::shared_ptr<DeviceContext> ctx) {
  LoopCloserCore core(set.maps, pipeline, std::move(ctx), "close_loops");
  LoopClosureResult out;
  out.corrected = set;
  const size_t K = set.frames.size();
  core.kf = &set.frames;
  // ---- the place index: every frame with points described once; the host copies are the queries
  std::vector<std::vector<uint8_t>> desc;
  for (size_t k = 0; k < K; k++) {
    if (!usable(set.frames[k])) continue;
    desc.push_back(core.describe(set.frames[k]));
    core.add(desc.back(), k);
  }
  core.frames.resize(K);
  for (size_t k = 0; k < K; k++) {
    std::copy(set.frames[k].pose, set.frames[k].pose + 12, core.frames[k].pose);
    core.frames[k].has_points = usable(set.frames[k]);
  }
  for (size_t q = 0; q < desc.size(); q++) core.frames[core.frame_of[q]].matches = core.search(desc[q]);
  core.s = path_lengths(core.frames);
  (void)loop_candidates(core.frames, core.opt, [&](const LoopPair& c) { return core.verify(c); });

  // ---- one optimisation over all frames
  if (!core.loops.empty()) {  // (otherwise the input, bit for bit)
    const std::vector<double> poses = core.optimize();
    for (size_t k = 0; k < K; k++) std::copy(&poses[12 * k], &poses[12 * k] + 12, out.corrected.frames[k].pose);
  }
  out.report = std::move(core.rep);
  return out;
}

// ================================================================== OnlineLoopCloser
OnlineLoopCloser::OnlineLoopCloser(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, std::shared_ptr<DeviceContext> ctx)
    : online_(OnlineLoopClosureOptions::FromConfig(pipeline)) {
  core_ = std::make_unique<LoopCloserCore>(maps, pipeline, std::move(ctx), "OnlineLoopCloser");
  core_->kf = &frames_;
}
OnlineLoopCloser::~OnlineLoopCloser() = default;
size_t OnlineLoopCloser::size() const { return raw_.size() / 12; }
const std::vector<double>& OnlineLoopCloser::rawPoses() const { return raw_; }
const std::vector<double>& OnlineLoopCloser::correctedPoses() const { return corrected_; }
const std::vector<PoseGraphEdge>& OnlineLoopCloser::loops() const { return core_->loops; }
const LoopReport& OnlineLoopCloser::report() const { return core_->rep; }

void OnlineLoopCloser::readFramesFrom(const std::vector<molahip_host::KeyFrame>* frames) {
  if (size() != 0) throw std::runtime_error("OnlineLoopCloser::readFramesFrom: frames have been pushed already");
  if (!frames) throw std::runtime_error("OnlineLoopCloser::readFramesFrom: no frames");
  external_ = frames;
  core_->kf = frames;
}

molahip_host::KeyFrameSet OnlineLoopCloser::rawKeyFrames() const {
  molahip_host::KeyFrameSet set;
  set.maps = core_->maps;
  set.frames.assign(core_->kf->begin(), core_->kf->begin() + (std::ptrdiff_t)size());
  for (size_t k = 0; k < set.frames.size(); k++) std::copy(&raw_[12 * k], &raw_[12 * k] + 12, set.frames[k].pose);
  return set;
}

OnlineLoopCloser::Step OnlineLoopCloser::push(molahip_host::KeyFrame frame) {
  if (external_) throw std::runtime_error("OnlineLoopCloser::push: the frames are read from the caller's vector (readFramesFrom); use pushStored");
  double raw[12];
  std::copy(frame.pose, frame.pose + 12, raw);
  frames_.push_back(std::move(frame));
  try {
    return push_frame(frames_.back(), raw);
  } catch (...) {
    frames_.pop_back();
    throw;
  }
}

OnlineLoopCloser::Step OnlineLoopCloser::pushStored(size_t index, const double raw_pose[12]) {
  if (!external_) throw std::runtime_error("OnlineLoopCloser::pushStored: no vector to read the frames from (readFramesFrom)");
  if (index != size() || index >= external_->size())
    throw std::runtime_error("OnlineLoopCloser::pushStored: frame " + std::to_string(index) + " is not the next one (" + std::to_string(size()) +
                             " pushed, " + std::to_string(external_->size()) + " stored)");
  return push_frame((*external_)[index], raw_pose);
}

// `f` is frame size() of the vector the core reads the layers from.  Nothing of the closer's state is kept when a device call throws:
// the same frame can be pushed again.
OnlineLoopCloser::Step OnlineLoopCloser::push_frame(const molahip_host::KeyFrame& f, const double raw[12]) {
  LoopCloserCore& c = *core_;
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(raw[k])) throw std::runtime_error("OnlineLoopCloser::push: non-finite pose");
  const size_t i = size();
  const size_t n_loops = c.loops.size(), n_pairs = c.rep.pairs.size(), n_points = n_with_points_;
  const LoopCandidateState state = state_;
  LoopFrame lf;
  std::copy(raw, raw + 12, lf.pose);
  lf.has_points = usable(f);
  c.s.push_back(i == 0 ? 0.0 : c.s[i - 1] + path_step(c.frames[i - 1].pose, raw));
  c.frames.push_back(std::move(lf));
  raw_.insert(raw_.end(), raw, raw + 12);
  Step step;
  try {
    std::vector<uint8_t> d;
    if (c.frames[i].has_points) {
      const bool checked = n_with_points_++ % online_.check_every_n_keyframes == 0;
      d = c.describe(f);
      if (checked) {
        c.frames[i].matches = c.search(d);  // the frames < i: the database as it stands before this frame's descriptor enters
        std::vector<LoopPair> tried;
        step.closed = loop_candidates_step(c.frames, c.s, i, c.opt, state_, [&](const LoopPair& p) { return c.verify(p); }, tried);
        step.pairs.assign(c.rep.pairs.begin() + (std::ptrdiff_t)n_pairs, c.rep.pairs.end());
        step.tried = !step.pairs.empty();
        std::vector<PlaceIndex::Match>().swap(c.frames[i].matches);  // (no later frame reads them)
      }
    }
    // the correction: from the raw chain and every loop so far, never from the previous correction -- what close_loops gives for
    // the frames pushed so far
    std::vector<double> corrected;
    if (!c.loops.empty()) corrected = c.optimize(step.closed);
    if (c.frames[i].has_points) c.add(d, i);  // (last: the database changes only when everything else has succeeded)
    if (c.loops.empty()) corrected_.insert(corrected_.end(), raw, raw + 12);
    else corrected_ = std::move(corrected);
  } catch (...) {
    c.s.pop_back();
    c.frames.pop_back();
    raw_.resize(12 * i);
    c.loops.resize(n_loops);
    c.rep.pairs.resize(n_pairs);
    state_ = state;
    n_with_points_ = n_points;
    throw;
  }
  return step;
}

LoopReport close_loops_file(const std::string& keyframe_file, const Config& pipeline, const std::string& output_keyframe_file,
                            std::shared_ptr<DeviceContext> ctx) {
  const LoopClosureResult r = close_loops(molahip_host::read_keyframe_file(keyframe_file), pipeline, std::move(ctx));
  molahip_host::write_keyframe_file(output_keyframe_file, r.corrected);
  return r.report;
}

}  // namespace mola_hip
