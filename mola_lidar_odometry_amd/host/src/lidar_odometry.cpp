// lidar_odometry.cpp -- see mola_lidar_odometry_hip/LidarOdometry.h.  Control logic only: the arithmetic on points
// is behind include/molahip.h.  Citations are module/src/LidarOdometry.cpp unless another file is named.
#include "mola_lidar_odometry_hip/LidarOdometry.h"
#include "mola_lidar_odometry_hip/LoopClosure.h"
#include "molahip_host/plugin_switches.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <set>
#include <mutex>
#include <thread>
#include <stdexcept>

namespace mola_hip {

using namespace mp2p_icp_hip;

namespace {

double to_double(const std::string& s) { return strtod(s.c_str(), nullptr); }
bool to_bool(const std::string& s) { return s == "true" || s == "True" || s == "1" || s == "yes"; }
constexpr double kDeg2Rad = M_PI / 180.0;

// "$f{expr}" (evaluated once, at object creation) or a plain number / expression
double eval_now(std::string s, const std::map<std::string, double>& vars) {
  if (s.size() > 4 && s.compare(0, 3, "$f{") == 0 && s.back() == '}') s = s.substr(3, s.size() - 4);
  return evaluate_expression(s, vars);
}

struct StageTimer {  // adds the wall time of its scope to a profile entry
  std::map<std::string, double>& prof;
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  StageTimer(std::map<std::string, double>& p, const char* n) : prof(p), name(n) {}
  ~StageTimer() { prof[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

std::string class_of(const Config& entry) { return entry["class_name"].asString(); }
bool ends_with(const std::string& s, const std::string& suffix) {
  return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

}  // namespace

// ================================================================== motion model
void NavStateFuse::initialize(const Config& c) {
  auto num = [&](const char* k, double& v) { if (c.has(k)) v = to_double(c[k].asString()); };
  num("max_time_to_use_velocity_model", max_time_to_use_velocity_model);
  num("sigma_random_walk_acceleration_linear", sigma_random_walk_acceleration_linear);
  num("sigma_random_walk_acceleration_angular", sigma_random_walk_acceleration_angular);
  if (c.has("motion_model_prior")) motion_model_prior = to_bool(c["motion_model_prior"].asString());
  initial_twist.reset();
  if (c.has("initial_twist") && c["initial_twist"].size() == 6) {
    double v[6];
    bool any = false;
    for (size_t i = 0; i < 6; i++) {
      v[i] = to_double(c["initial_twist"].at(i).asString());
      any = any || v[i] != 0.0;
    }
    if (any) {
      Twist tw;
      tw.vx = v[0]; tw.vy = v[1]; tw.vz = v[2]; tw.wx = v[3]; tw.wy = v[4]; tw.wz = v[5];
      initial_twist = tw;
    }
  }
  reset();
}
void NavStateFuse::reset() {
  last_pose_.reset();
  twist_.reset();
  last_t_ = 0;
  for (double& v : last_cov_) v = 0;
}
void NavStateFuse::fuse_pose(double t, const CPose3D& pose, const double* cov) {
  if (last_pose_) {
    const double dt = t - last_t_;
    if (dt > 0 && dt <= max_time_to_use_velocity_model) {
      const CPose3D incr = pose - *last_pose_;  // increment in the frame of the previous pose
      double w[3];
      incr.so3Log(w);
      Twist tw;
      tw.vx = incr.T[3] / dt; tw.vy = incr.T[7] / dt; tw.vz = incr.T[11] / dt;
      tw.wx = w[0] / dt; tw.wy = w[1] / dt; tw.wz = w[2] / dt;
      twist_ = tw;
    } else {
      twist_.reset();  // a gap or a stamp that does not advance: no velocity from this pair
    }
  } else if (initial_twist) {
    twist_ = initial_twist;
  }
  last_pose_ = pose;
  for (int i = 0; i < 36; i++) last_cov_[i] = cov ? cov[i] : ((i % 7 == 0) ? 1e-12 : 0.0);  // (:834-836: "cannot be zero")
  last_t_ = t;
}

void NavStateFuse::rebase(const CPose3D& delta) {
  if (last_pose_) last_pose_ = delta + *last_pose_;
}

namespace {
// inverse of a symmetric positive-definite 6x6 (Cholesky); false when it is not
bool spd_inverse6(const double* A, double* Ainv) {
  double L[36] = {0};
  for (int i = 0; i < 6; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; k++) s -= L[i * 6 + k] * L[j * 6 + k];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[i * 6 + i] = std::sqrt(s);
      } else {
        L[i * 6 + j] = s / L[j * 6 + j];
      }
    }
  double Li[36] = {0};  // inverse of the lower-triangular factor
  for (int c = 0; c < 6; c++) {
    Li[c * 6 + c] = 1.0 / L[c * 6 + c];
    for (int r = c + 1; r < 6; r++) {
      double s = 0;
      for (int k = c; k < r; k++) s -= L[r * 6 + k] * Li[k * 6 + c];
      Li[r * 6 + c] = s / L[r * 6 + r];
    }
  }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0;
      for (int k = 0; k < 6; k++) s += Li[k * 6 + i] * Li[k * 6 + j];
      Ainv[i * 6 + j] = s;
    }
  return true;
}
}  // namespace

std::optional<NavStateFuse::NavState> NavStateFuse::estimated_navstate(double t) const {
  if (!last_pose_ || !twist_) return std::nullopt;
  const double dt = t - last_t_;
  if (dt < 0 || dt > max_time_to_use_velocity_model) return std::nullopt;
  const double w[3] = {twist_->wx * dt, twist_->wy * dt, twist_->wz * dt};
  const double v[3] = {twist_->vx * dt, twist_->vy * dt, twist_->vz * dt};
  NavState ns;
  ns.pose.mean = *last_pose_ + CPose3D::FromRotVecAndTranslation(w, v);
  ns.twist = *twist_;
  if (motion_model_prior) {
    // covariance of the last pose, grown by the random-walk acceleration over dt, in the solver's tangent order:
    // (x,y,z,yaw,pitch,roll) -> [v; w] with w = (roll, pitch, yaw) to first order
    static const int perm[6] = {0, 1, 2, 5, 4, 3};
    double C[36];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) C[i * 6 + j] = last_cov_[perm[i] * 6 + perm[j]];
    const double sl = sigma_random_walk_acceleration_linear * dt, sa = sigma_random_walk_acceleration_angular * dt;
    for (int i = 0; i < 3; i++) C[i * 7] += sl * sl;
    for (int i = 3; i < 6; i++) C[i * 7] += sa * sa;
    double Ci[36];
    if (spd_inverse6(C, Ci))
      for (int i = 0; i < 36; i++) ns.pose.cov_inv[i] = Ci[i];
  }
  return ns;
}

// ================================================================== key-frame list
std::pair<bool, CPose3D> SearchablePoseList::check(const CPose3D& p) const {
  if (poses_.empty()) return {true, CPose3D()};
  size_t best = 0;
  double best_d2 = INFINITY;
  for (size_t i = 0; i < poses_.size(); i++) {
    const double dx = poses_[i].T[3] - p.T[3], dy = poses_[i].T[7] - p.T[7], dz = poses_[i].T[11] - p.T[11];
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < best_d2) {
      best_d2 = d2;
      best = i;
    }
  }
  return {false, p - poses_[best]};
}
void SearchablePoseList::removeAllFartherThan(const CPose3D& p, double max_dist) {
  std::vector<CPose3D> kept;
  for (const auto& q : poses_) {
    const double dx = q.T[3] - p.T[3], dy = q.T[7] - p.T[7], dz = q.T[11] - p.T[11];
    if (std::sqrt(dx * dx + dy * dy + dz * dz) <= max_dist) kept.push_back(q);
  }
  poses_.swap(kept);
}

// ================================================================== key-frames of the session
KeyFrameStore::Verdict KeyFrameStore::decide(bool first_scan, bool icp_good, const CPose3D& pose, double min_translation,
                                             double min_rotation_deg, bool add_non_keyframes_too) {
  Verdict v;
  if (first_scan) {  // (:817-824: a key-frame with its points; the checker is not touched)
    v.stored = v.keyframe = true;
    return v;
  }
  if (!icp_good) return v;
  bool is_first;
  CPose3D d;
  if (last_only_) {
    is_first = !last_.has_value();
    if (!is_first) d = pose - *last_;
  } else {
    std::tie(is_first, d) = all_.check(pose);
  }
  const bool enough = is_first || d.translationNorm() > min_translation || d.rotationAngle() > min_rotation_deg * kDeg2Rad;
  v.keyframe = enough;
  v.stored = enough || add_non_keyframes_too;
  if (enough) {
    if (last_only_) last_ = pose;
    else all_.insert(pose);
    in_checker_.push_back(set_.frames.size());
  }
  return v;
}

void KeyFrameStore::reset(const molahip_host::KeyFrameSet& initial) {
  all_.clear();
  last_.reset();
  in_checker_.clear();
  set_ = initial;
}

void KeyFrameStore::setPoses(const std::vector<double>& poses) {
  if (poses.size() != 12 * set_.frames.size())
    throw std::runtime_error("KeyFrameStore::setPoses: " + std::to_string(poses.size()) + " values for " + std::to_string(set_.frames.size()) + " frames");
  for (size_t k = 0; k < set_.frames.size(); k++) std::copy(&poses[12 * k], &poses[12 * k] + 12, set_.frames[k].pose);
  all_.clear();
  last_.reset();
  for (size_t k : in_checker_) {
    if (k >= set_.frames.size()) continue;
    CPose3D p;
    std::copy(set_.frames[k].pose, set_.frames[k].pose + 12, p.T);
    if (last_only_) last_ = p;
    else all_.insert(p);
  }
}

std::vector<mp2p_icp_hip::PosedFrame> session_map_frames(const molahip_host::KeyFrameSet& set, size_t map_index,
                                                         const std::function<bool(const molahip_host::KeyFrame&)>& keep) {
  std::vector<mp2p_icp_hip::PosedFrame> frames;
  for (const auto& f : set.frames) {
    if (!f.has_points || (keep && !keep(f))) continue;
    for (const auto& l : f.layers) {  // frame order, then step order
      if (l.map_index != map_index) continue;
      mp2p_icp_hip::PosedFrame pf;
      pf.x = l.x.data(); pf.y = l.y.data(); pf.z = l.z.data();
      pf.n = l.x.size();
      std::copy(f.pose, f.pose + 12, pf.pose.T);
      frames.push_back(pf);
    }
  }
  return frames;
}

std::vector<molahip_host::LocalMapRecord> build_session_maps(const molahip_host::KeyFrameSet& set, std::shared_ptr<DeviceContext> ctx,
                                                             uint64_t max_points_per_pass) {
  for (const auto& t : set.maps) {
    if (t.class_name == "CVoxelMap")
      throw std::runtime_error("build_session_maps: target map '" + t.name + "' is a '" + t.class_name + "': an occupancy map has no snapshot, so "
                               "no session map can be built from its key-frames (HashedVoxelPointCloud, NDT and SparseTreesPointCloud can)");
    if (!molahip_host::local_map_class_known(t.class_name))
      throw std::runtime_error("build_session_maps: target map '" + t.name + "' is of the unknown class '" + t.class_name +
                               "' (HashedVoxelPointCloud, NDT and SparseTreesPointCloud can be built)");
  }
  if (!ctx) ctx = DeviceContext::Default();
  std::vector<molahip_host::LocalMapRecord> out;
  for (size_t k = 0; k < set.maps.size(); k++) {
    const auto& t = set.maps[k];
    molahip_host::LocalMapRecord empty;
    empty.name = t.name;
    empty.class_name = t.class_name;
    empty.params = t.params;
    empty.remove_voxels_farther_than = t.remove_voxels_farther_than;
    auto map = mp2p_icp_hip::make_local_map(empty, ctx);
    map->insertFrames(session_map_frames(set, k), max_points_per_pass);
    out.push_back(map->snapshot(t.name, t.remove_voxels_farther_than));
  }
  return out;
}

std::vector<molahip_host::LocalMapRecord> build_session_maps(const std::string& keyframe_file, std::shared_ptr<DeviceContext> ctx,
                                                             uint64_t max_points_per_pass) {
  return build_session_maps(molahip_host::read_keyframe_file(keyframe_file), std::move(ctx), max_points_per_pass);
}

void build_session_map_file(const molahip_host::KeyFrameSet& frames, const std::string& local_map_file, std::shared_ptr<DeviceContext> ctx,
                            uint64_t max_points_per_pass) {
  molahip_host::write_local_map_file(local_map_file, build_session_maps(frames, std::move(ctx), max_points_per_pass));
}

// ================================================================== parameters
void LidarOdometry::Params::load_from(const Config& c) {
  auto num = [&](const Config& n, const char* k, double& v) { if (n.has(k)) v = to_double(n[k].asString()); };
  auto flag = [&](const Config& n, const char* k, bool& v) { if (n.has(k)) v = to_bool(n[k].asString()); };
  num(c, "min_time_between_scans", min_time_between_scans);
  num(c, "max_sensor_range_filter_coefficient", max_sensor_range_filter_coefficient);
  num(c, "absolute_minimum_sensor_range", absolute_minimum_sensor_range);
  flag(c, "optimize_twist", optimize_twist);
  num(c, "optimize_twist_rerun_min_trans", optimize_twist_rerun_min_trans);
  num(c, "optimize_twist_rerun_min_rot_deg", optimize_twist_rerun_min_rot_deg);
  if (c.has("optimize_twist_max_corrections"))
    optimize_twist_max_corrections = (size_t)to_double(c["optimize_twist_max_corrections"].asString());
  num(c, "min_icp_goodness", min_icp_goodness);
  if (c.has("local_map_updates")) {
    const Config& l = c["local_map_updates"];
    flag(l, "enabled", local_map_updates_enabled);
    // DECLARE_PARAMETER_IN_REQ: formulas over wx,wy,wz and ESTIMATED_SENSOR_MAX_RANGE (yaml:44-46)
    parameterFromConfig(l, "min_translation_between_keyframes", &min_translation_between_keyframes, true);
    parameterFromConfig(l, "min_rotation_between_keyframes", &min_rotation_between_keyframes, true);
    parameterFromConfig(l, "max_distance_to_keep_keyframes", &max_distance_to_keep_keyframes, false);
    if (l.has("check_for_removal_every_n")) check_for_removal_every_n = (uint32_t)to_double(l["check_for_removal_every_n"].asString());
    load_existing_local_map.clear();
    if (l.has("load_existing_local_map") && !l["load_existing_local_map"].isNull()) {
      std::string f = l["load_existing_local_map"].asString();
      if (f.size() >= 2 && (f.front() == '"' || f.front() == '\'') && f.back() == f.front()) f = f.substr(1, f.size() - 2);  // (${MOLA_LOAD_MM|""})
      load_existing_local_map = f;
    }
  }
  simplemap = SimpleMapOptions();
  if (c.has("simplemap")) {
    const Config& m = c["simplemap"];
    auto text = [&](const char* k, std::string& v) {
      if (!m.has(k) || m[k].isNull()) return;
      std::string f = m[k].asString();
      if (f.size() >= 2 && (f.front() == '"' || f.front() == '\'') && f.back() == f.front()) f = f.substr(1, f.size() - 2);  // (${MOLA_LOAD_SM|""})
      v = f;
    };
    flag(m, "generate", simplemap.generate);
    // DECLARE_PARAMETER_IN_OPT: formulas over wx,wy,wz and ESTIMATED_SENSOR_MAX_RANGE (yaml:71-72), realised with local_map_updates'
    parameterFromConfig(m, "min_translation_between_keyframes", &simplemap.min_translation_between_keyframes, false);
    parameterFromConfig(m, "min_rotation_between_keyframes", &simplemap.min_rotation_between_keyframes, false);
    flag(m, "measure_from_last_kf_only", simplemap.measure_from_last_kf_only);
    flag(m, "add_non_keyframes_too", simplemap.add_non_keyframes_too);
    flag(m, "generate_lazy_load_scan_files", simplemap.generate_lazy_load_scan_files);
    num(m, "save_gnss_max_age", simplemap.save_gnss_max_age);  // (read and ignored: there is no GNSS input)
    text("save_final_map_to_file", simplemap.save_final_map_to_file);
    text("load_existing_simple_map", simplemap.load_existing_simple_map);
  }
  if (c.has("adaptive_threshold")) {
    const Config& a = c["adaptive_threshold"];
    flag(a, "enabled", adaptive_threshold_enabled);
    num(a, "initial_sigma", initial_sigma);
    num(a, "min_motion", min_motion);
    num(a, "maximum_sigma", maximum_sigma);
    num(a, "kp", kp);
    num(a, "alpha", alpha);
  }
  if (c.has("observation_validity_checks")) {
    const Config& v = c["observation_validity_checks"];
    flag(v, "enabled", validity_check_enabled);
    if (v.has("minimum_point_count")) validity_minimum_point_count = (uint32_t)to_double(v["minimum_point_count"].asString());
  }
  if (c.has("multiple_lidars")) {
    const Config& m = c["multiple_lidars"];
    if (m.has("lidar_count")) lidar_count = (uint32_t)to_double(m["lidar_count"].asString());
    num(m, "max_time_offset", max_time_offset);
  }
  // a scalar or a sequence of regular expressions (:261-275).  The reference insists on the key; the pipeline files of this
  // driver have lived without it, so here its absence means "every label".
  lidar_sensor_labels.clear();
  if (c.has("lidar_sensor_labels")) {
    const Config& l = c["lidar_sensor_labels"];
    if (l.kind == Config::Kind::Seq)
      for (size_t i = 0; i < l.size(); i++) lidar_sensor_labels.push_back(l.at(i).asString());
    else if (!l.isNull())
      lidar_sensor_labels.push_back(l.asString());
  }
}

// ================================================================== rigs: the grouping rule
std::optional<SensorSync::Group> SensorSync::push(const std::string& label, double stamp) {
  if (lidar_count_ <= 1) {  // single LiDAR (:686-689): no waiting set, no window
    Group g;
    g.labels = {label};
    g.stamps = {stamp};
    g.dts = {0.0};
    return g;
  }
  waiting_[label] = stamp;  // (:668)
  if (waiting_.size() < lidar_count_) return std::nullopt;
  Group g;
  for (const auto& [l, t] : waiting_) {  // label order (:674-679)
    if (std::abs(t - stamp) > max_time_offset_) {
      g.discarded.push_back(l);
      continue;
    }
    g.labels.push_back(l);
    g.stamps.push_back(t);
    g.dts.push_back(t - g.stamps.front());  // relative to the first KEPT observation in label order (:702, 711)
  }
  waiting_.clear();  // (:681)
  return g;
}

std::vector<std::string> SensorSync::waiting() const {
  std::vector<std::string> l;
  for (const auto& kv : waiting_) l.push_back(kv.first);
  return l;
}

// The observation filter chain the device implements, recognised from the pipeline file:
//   1st pass  Decimate(raw -> A) -> [ByRange(A -> B)] -> [BoundingBox(B -> C)] -> Decimate(C -> D)      (yaml:278-319)
//   2nd pass  [DeleteLayer] -> Deskew(C -> for_map) -> Deskew(D -> for_icp)                               (yaml:322-350)
//   merge     FilterMerge(for_map -> local map layer)                                                     (yaml:362-368)
struct LidarOdometry::FilterPlan : public Parameterizable {
  double decim_map_res = 0, decim_icp_res = 0, range_min = 0, range_max = 0;
  double bbox_min[3] = {0, 0, 0}, bbox_max[3] = {0, 0, 0};
  double time_offset = 0;
  uint32_t min_points_to_filter = 0;
  int32_t decim_map_method = MH_DECIMATE_FIRST_POINT, decim_icp_method = MH_DECIMATE_FIRST_POINT;
  int32_t bbox_mode = MH_BBOX_OFF, timestamp_method = MH_TS_NONE;
  bool skip_deskew = false;
  std::string layer_for_map, layer_for_icp, map_layer;

  static void unsupported(const std::string& what) {
    throw std::runtime_error("LidarOdometry (HIP): unsupported observation filter chain: " + what +
                             ". Implemented on the device: FilterAdjustTimestamps; FilterDecimateVoxels(FirstPoint | ClosestToAverage) -> "
                             "[FilterByRange] -> [FilterBoundingBox] -> FilterDecimateVoxels(FirstPoint | ClosestToAverage); FilterDeskew x2; "
                             "FilterMerge (the chain of pipelines/lidar3d-default.yaml)");
  }
  void decimate(const Config& p, double* res) {
    int32_t method = MH_DECIMATE_FIRST_POINT;  // (the default of FilterDecimateVoxels; lidar3d-default.yaml:291 spells it out)
    if (p.has("decimate_method")) {
      const std::string m = p["decimate_method"].asString();
      if (ends_with(m, "ClosestToAverage")) method = MH_DECIMATE_CLOSEST_TO_AVERAGE;  // (yaml:292, the commented alternative)
      else if (!ends_with(m, "FirstPoint")) unsupported("decimate_method " + m);
    }
    (res == &decim_map_res ? decim_map_method : decim_icp_method) = method;
    parameterFromConfig(p, "voxel_filter_resolution", res, true);
    const uint32_t mp = p.has("minimum_input_points_to_filter") ? (uint32_t)to_double(p["minimum_input_points_to_filter"].asString()) : 0;
    if (res == &decim_map_res) min_points_to_filter = mp;
    else if (mp != min_points_to_filter) unsupported("different minimum_input_points_to_filter in the two decimations");
  }
  void load(const Config& cfg) {
    if (cfg.has("observations_filter_adjust_timestamps")) {
      const Config& s = cfg["observations_filter_adjust_timestamps"];
      for (size_t i = 0; i < s.size(); i++) {
        if (!ends_with(class_of(s.at(i)), "FilterAdjustTimestamps")) unsupported(class_of(s.at(i)));
        const Config& p = s.at(i)["params"];
        const std::string m = p.getOr("method", "TimestampAdjustMethod::MiddleIsZero");
        timestamp_method = ends_with(m, "MiddleIsZero") ? MH_TS_MIDDLE_IS_ZERO : ends_with(m, "EarliestIsZero") ? MH_TS_EARLIEST_IS_ZERO : -1;
        if (timestamp_method < 0) unsupported("timestamp method " + m);
        if (p.has("time_offset")) parameterFromConfig(p, "time_offset", &time_offset, false);
      }
    }
    // ---- 1st pass
    const Config& f1 = cfg["observations_filter_1st_pass"];
    std::string cur = "raw";
    size_t i = 0;
    auto params_of = [&](size_t k) -> const Config& { return f1.at(k)["params"]; };
    if (i >= f1.size() || !ends_with(class_of(f1.at(i)), "FilterDecimateVoxels")) unsupported("1st pass must start with FilterDecimateVoxels");
    if (params_of(i)["input_pointcloud_layer"].asString() != cur) unsupported("first decimation must read layer 'raw'");
    decimate(params_of(i), &decim_map_res);
    cur = params_of(i)["output_pointcloud_layer"].asString();
    i++;
    if (i < f1.size() && ends_with(class_of(f1.at(i)), "FilterByRange")) {
      const Config& p = params_of(i);
      if (p["input_pointcloud_layer"].asString() != cur || !p.has("output_layer_between")) unsupported("FilterByRange wiring");
      parameterFromConfig(p, "range_min", &range_min, true);
      parameterFromConfig(p, "range_max", &range_max, true);
      cur = p["output_layer_between"].asString();
      i++;
    }
    if (i < f1.size() && ends_with(class_of(f1.at(i)), "FilterBoundingBox")) {
      const Config& p = params_of(i);
      if (p["input_pointcloud_layer"].asString() != cur) unsupported("FilterBoundingBox wiring");
      if (p.has("outside_pointcloud_layer")) { bbox_mode = MH_BBOX_KEEP_OUTSIDE; cur = p["outside_pointcloud_layer"].asString(); }
      else if (p.has("inside_pointcloud_layer")) { bbox_mode = MH_BBOX_KEEP_INSIDE; cur = p["inside_pointcloud_layer"].asString(); }
      else unsupported("FilterBoundingBox without an output layer");
      for (int a = 0; a < 3; a++) {
        declareParameter("bounding_box_min", p["bounding_box_min"].at(a).asString(), &bbox_min[a]);
        declareParameter("bounding_box_max", p["bounding_box_max"].at(a).asString(), &bbox_max[a]);
      }
      i++;
    }
    const std::string skewed_map = cur;
    if (i >= f1.size() || !ends_with(class_of(f1.at(i)), "FilterDecimateVoxels")) unsupported("1st pass must end with FilterDecimateVoxels");
    if (params_of(i)["input_pointcloud_layer"].asString() != cur) unsupported("second decimation wiring");
    decimate(params_of(i), &decim_icp_res);
    const std::string skewed_icp = params_of(i)["output_pointcloud_layer"].asString();
    if (++i != f1.size()) unsupported("extra filters after the second decimation: " + class_of(f1.at(i)));
    // ---- 2nd pass
    const Config& f2 = cfg["observations_filter_2nd_pass"];
    for (size_t k = 0; k < f2.size(); k++) {
      const std::string cn = class_of(f2.at(k));
      if (ends_with(cn, "FilterDeleteLayer")) continue;
      if (!ends_with(cn, "FilterDeskew")) unsupported(cn);
      const Config& p = f2.at(k)["params"];
      const std::string in = p["input_pointcloud_layer"].asString(), out = p["output_pointcloud_layer"].asString();
      if (in == skewed_map) layer_for_map = out;
      else if (in == skewed_icp) layer_for_icp = out;
      else unsupported("FilterDeskew reads unknown layer " + in);
      if (p.has("skip_deskew")) skip_deskew = to_bool(p["skip_deskew"].asString());
    }
    if (layer_for_map.empty() || layer_for_icp.empty()) unsupported("both skewed layers need a FilterDeskew");
    // ---- merge
    const Config& mg = cfg["insert_observation_into_local_map"];
    if (mg.size() != 1 || !ends_with(class_of(mg.at(0)), "FilterMerge")) unsupported("insert_observation_into_local_map must be one FilterMerge");
    const Config& mp = mg.at(0)["params"];
    if (mp["input_pointcloud_layer"].asString() != layer_for_map) unsupported("FilterMerge must read the de-skewed map layer");
    if (mp.has("input_layer_in_local_coordinates") && !to_bool(mp["input_layer_in_local_coordinates"].asString()))
      unsupported("FilterMerge with input_layer_in_local_coordinates: false");
    map_layer = mp["target_layer"].asString();
  }
};

// Any other chain of the filters the device implements (extras/lidar3d-edges.yaml, -dual-map, -kissicp-like, -near-far):
// ordered steps of the two passes over a name -> layer table, one device map per localmap_generator entry, one FilterMerge
// per (layer, map).  Each step maps onto one entry point:
//   FilterDeskew -> mh_scan_deskew; FilterByRange (output_layer_between) / FilterBoundingBox (inside and / or outside) /
//   FilterDecimateVoxels -> mh_scan_preprocess with the other stages skipped; FilterCurvature -> mh_scan_curvature;
//   FilterDeleteLayer -> the layer leaves the table; observations_filter_adjust_timestamps -> mh_scan_preprocess on 'raw'
//   with every filter stage skipped (it keeps the finite points, as every preprocess call does);
//   with setIntensityInput(true) (extras/lidar3d-intensity.yaml): FilterNormalizeIntensity -> mh_scan_normalize_intensity in
//   place, 1st pass only; FilterByIntensity -> mh_scan_by_intensity.
//   observations_generator (rgbd.yaml:226-244): absent or a plain Generator -> the observation is the point layer 'raw';
//   GeneratorEdgesFromRangeImage -> the observation is a depth image (onDepthImage) that mh_scan_edges_from_range_image turns
//   into target_layer and planes_target_layer when it is uploaded -- the only layers the passes start from, there is no 'raw'.
struct LidarOdometry::GeneralPlan : public Parameterizable {
  enum class Kind { Deskew, Preprocess, Curvature, Delete, NormalizeIntensity, ByIntensity, EdgesFromRangeImage };
  struct Step {
    Kind kind = Kind::Delete;
    int pass = 1;
    std::string cls, in;
    std::vector<std::string> out;  // Deskew / Preprocess: 1; Curvature: larger, smaller, other ("" = not asked for); Delete: names
    double res = 0, range_min = 0, range_max = 0, bbox_min[3] = {0, 0, 0}, bbox_max[3] = {0, 0, 0};
    int32_t method = MH_DECIMATE_FIRST_POINT, bbox_mode = MH_BBOX_OFF;
    uint32_t min_points = 0;
    bool range_on = false;
    double max_cosine = 0, min_clearance = 0, max_gap = 0;
    bool skip_deskew = false;
    double low_threshold = 0, high_threshold = 0;  // ByIntensity
    bool remember_range = false;                   // NormalizeIntensity: remember_intensity_range
    float range[2] = {NAN, NAN};                   // ... the remembered {min, max} (reset() forgets it)
    uint32_t row_window_length = 0;                // EdgesFromRangeImage (pass 0: it runs when the image is uploaded)
    double score_threshold = 0;
  };
  struct MapSlot {
    std::string name;
    Config def;
    std::shared_ptr<HashedVoxelPointCloud> map;  // created at the first key-frame (its $f{} formulas need the sensor range)
    float remove_far = 0.f;
    double voxel_size = 0;
  };
  std::deque<Step> steps;  // (a deque: the formulas are bound to the steps' fields by address)
  bool intensity_input = false;  // LidarOdometry::setIntensityInput: intensity filters are accepted
  bool reads_intensity = false;  // an intensity filter is among the steps: 'raw' carries the channel
  bool depth_input = false;      // observations_generator is a GeneratorEdgesFromRangeImage: steps[0] is its step
  bool has_2nd_pass = false;     // any step of observations_filter_2nd_pass
  float gen_bb_min[3] = {0, 0, 0}, gen_bb_max[3] = {0, 0, 0};  // depth_input: union bounding box of the generator's layers
  int32_t timestamp_method = MH_TS_NONE;
  double time_offset = 0;
  std::vector<MapSlot> maps;
  std::vector<std::pair<std::string, size_t>> merges;  // layer -> index in maps
  // per-scan state: every layer name's buffer (reused scan after scan), the layers alive after pass 1 / now
  std::map<std::string, std::shared_ptr<DevicePointCloud>> buf;
  std::shared_ptr<DevicePointCloud> raw_adjusted;
  std::set<std::string> alive_1st, alive;

  static void unsupported(const std::string& what) {
    throw std::runtime_error("LidarOdometry (HIP): unsupported observation filter chain: " + what +
                             ". Implemented on the device: the chain of pipelines/lidar3d-default.yaml, and chains over named "
                             "layers of FilterAdjustTimestamps, FilterDeskew, FilterByRange(output_layer_between), "
                             "FilterBoundingBox, FilterDecimateVoxels(FirstPoint | ClosestToAverage), FilterCurvature, "
                             "FilterDeleteLayer, FilterNormalizeIntensity and FilterByIntensity (with setIntensityInput), "
                             "and FilterMerge into HashedVoxelPointCloud / NDT / CVoxelMap / SparseTreesPointCloud maps; "
                             "observations_generator: Generator (point clouds) or GeneratorEdgesFromRangeImage (depth images)");
  }
  // observations_generator names a GeneratorEdgesFromRangeImage (such a file always takes the general plan)
  static bool wants_depth_input(const Config& cfg) {
    if (!cfg.has("observations_generator")) return false;
    const Config& gen = cfg["observations_generator"];
    for (size_t i = 0; i < gen.size(); i++)
      if (ends_with(class_of(gen.at(i)), "GeneratorEdgesFromRangeImage")) return true;
    return false;
  }
  static std::vector<std::string> names_of(const Config& c) {
    std::vector<std::string> v;
    if (c.kind == Config::Kind::Seq)
      for (size_t i = 0; i < c.size(); i++) v.push_back(c.at(i).asString());
    else if (!c.isNull())
      v.push_back(c.asString());
    return v;
  }
  void load_pass(const Config& f, int pass, std::set<std::string>& known) {
    for (size_t k = 0; k < f.size(); k++) {
      const std::string cn = class_of(f.at(k));
      const Config& p = f.at(k)["params"];
      steps.emplace_back();  // (declared formulas point into the step: it is built in place)
      Step& st = steps.back();
      st.pass = pass;
      st.cls = cn;
      auto input = [&]() {
        st.in = p.getOr("input_pointcloud_layer", "");
        if (!known.count(st.in)) unsupported(cn + " reads layer '" + st.in + "', which no earlier filter writes");
      };
      auto output = [&](const std::string& o) {
        if (o.empty()) unsupported(cn + " without an output layer");
        if (o == st.in) unsupported(cn + " writes its own input layer '" + o + "'");
        if (o == "raw") unsupported(cn + " writes layer 'raw'");
        st.out.push_back(o);
      };
      if (ends_with(cn, "FilterDeleteLayer")) {
        st.kind = Kind::Delete;
        st.out = names_of(p["pointcloud_layer_to_remove"]);
        for (const auto& n : st.out) known.erase(n);
      } else if (ends_with(cn, "FilterDeskew")) {
        st.kind = Kind::Deskew;
        input();
        output(p.getOr("output_pointcloud_layer", ""));
        if (p.has("skip_deskew")) st.skip_deskew = to_bool(p["skip_deskew"].asString());
      } else if (ends_with(cn, "FilterByRange")) {
        st.kind = Kind::Preprocess;
        input();
        if (!p.has("output_layer_between") || p.has("output_layer_outside")) unsupported("FilterByRange other than output_layer_between");
        if (p.has("center")) unsupported("FilterByRange with a center");
        output(p["output_layer_between"].asString());
        st.range_on = true;
        parameterFromConfig(p, "range_min", &st.range_min, true);
        parameterFromConfig(p, "range_max", &st.range_max, true);
      } else if (ends_with(cn, "FilterBoundingBox")) {
        input();
        const bool in_l = p.has("inside_pointcloud_layer"), out_l = p.has("outside_pointcloud_layer");
        if (!in_l && !out_l) unsupported("FilterBoundingBox without an output layer");
        const Step proto = st;
        steps.pop_back();  // one step per output layer
        for (int mode : {MH_BBOX_KEEP_INSIDE, MH_BBOX_KEEP_OUTSIDE}) {
          if (!(mode == MH_BBOX_KEEP_INSIDE ? in_l : out_l)) continue;
          steps.push_back(proto);
          Step& b = steps.back();
          b.kind = Kind::Preprocess;
          b.bbox_mode = mode;
          const std::string o = p[mode == MH_BBOX_KEEP_INSIDE ? "inside_pointcloud_layer" : "outside_pointcloud_layer"].asString();
          if (o.empty() || o == b.in || o == "raw") unsupported("FilterBoundingBox output layer '" + o + "'");
          b.out = {o};
          for (int a = 0; a < 3; a++) {
            declareParameter("bounding_box_min", p["bounding_box_min"].at(a).asString(), &b.bbox_min[a]);
            declareParameter("bounding_box_max", p["bounding_box_max"].at(a).asString(), &b.bbox_max[a]);
          }
          known.insert(o);
        }
        continue;
      } else if (ends_with(cn, "FilterDecimateVoxels")) {
        st.kind = Kind::Preprocess;
        input();
        output(p.getOr("output_pointcloud_layer", ""));
        if (p.has("decimate_method")) {
          const std::string m = p["decimate_method"].asString();
          if (ends_with(m, "ClosestToAverage")) st.method = MH_DECIMATE_CLOSEST_TO_AVERAGE;
          else if (!ends_with(m, "FirstPoint")) unsupported("decimate_method " + m);
        }
        if (p.has("minimum_input_points_to_filter")) st.min_points = (uint32_t)to_double(p["minimum_input_points_to_filter"].asString());
        parameterFromConfig(p, "voxel_filter_resolution", &st.res, true);
      } else if (ends_with(cn, "FilterCurvature")) {
        st.kind = Kind::Curvature;
        input();
        const char* keys[3] = {"output_layer_larger_curvature", "output_layer_smaller_curvature", "output_layer_other"};
        for (const char* key : keys) {
          const std::string o = p.getOr(key, "");
          if (o.empty()) st.out.push_back("");
          else output(o);
        }
        if (st.out[0].empty() && st.out[1].empty() && st.out[2].empty()) unsupported("FilterCurvature without an output layer");
        if ((!st.out[0].empty() && (st.out[0] == st.out[1] || st.out[0] == st.out[2])) || (!st.out[1].empty() && st.out[1] == st.out[2]))
          unsupported("FilterCurvature writes one layer twice");
        parameterFromConfig(p, "max_cosine", &st.max_cosine, true);
        parameterFromConfig(p, "min_clearance", &st.min_clearance, true);
        parameterFromConfig(p, "max_gap", &st.max_gap, true);
      } else if (ends_with(cn, "Intensity") && !intensity_input) {
        unsupported(cn + " (the observations carry no intensity: LidarOdometry::setIntensityInput(true) declares it)");
      } else if (ends_with(cn, "FilterNormalizeIntensity")) {
        // (the twist hook re-runs the 2nd pass from the same start: an in-place normalisation there, with its remembered
        //  range, would be applied twice)
        if (pass != 1) unsupported(cn + " in observations_filter_2nd_pass (it normalises in place, and the twist hook re-runs that pass)");
        st.kind = Kind::NormalizeIntensity;
        st.in = p.getOr("pointcloud_layer", "");
        if (!known.count(st.in)) unsupported(cn + " reads layer '" + st.in + "', which no earlier filter writes");
        if (p.has("remember_intensity_range")) st.remember_range = to_bool(p["remember_intensity_range"].asString());
        reads_intensity = true;
      } else if (ends_with(cn, "FilterByIntensity")) {
        st.kind = Kind::ByIntensity;
        input();
        const char* keys[3] = {"output_layer_low_intensity", "output_layer_mid_intensity", "output_layer_high_intensity"};
        for (const char* key : keys) {
          const std::string o = p.getOr(key, "");
          if (o.empty()) st.out.push_back("");
          else output(o);
        }
        if (st.out[0].empty() && st.out[1].empty() && st.out[2].empty()) unsupported("FilterByIntensity without an output layer");
        if ((!st.out[0].empty() && (st.out[0] == st.out[1] || st.out[0] == st.out[2])) || (!st.out[1].empty() && st.out[1] == st.out[2]))
          unsupported("FilterByIntensity writes one layer twice");
        parameterFromConfig(p, "low_threshold", &st.low_threshold, true);
        parameterFromConfig(p, "high_threshold", &st.high_threshold, true);
        reads_intensity = true;
      } else {
        unsupported(cn);
      }
      if (st.kind != Kind::Delete)
        for (const auto& o : st.out)
          if (!o.empty()) known.insert(o);
    }
  }
  void load(const Config& cfg) {
    if (cfg.has("observations_filter_adjust_timestamps")) {
      const Config& s = cfg["observations_filter_adjust_timestamps"];
      for (size_t i = 0; i < s.size(); i++) {
        if (!ends_with(class_of(s.at(i)), "FilterAdjustTimestamps")) unsupported(class_of(s.at(i)));
        const Config& p = s.at(i)["params"];
        if (p.getOr("pointcloud_layer", "raw") != "raw") unsupported("FilterAdjustTimestamps on a layer other than 'raw'");
        const std::string m = p.getOr("method", "TimestampAdjustMethod::MiddleIsZero");
        timestamp_method = ends_with(m, "MiddleIsZero") ? MH_TS_MIDDLE_IS_ZERO : ends_with(m, "EarliestIsZero") ? MH_TS_EARLIEST_IS_ZERO : -1;
        if (timestamp_method < 0) unsupported("timestamp method " + m);
        if (p.has("time_offset")) parameterFromConfig(p, "time_offset", &time_offset, false);
      }
    }
    std::set<std::string> known = {"raw"};
    if (cfg.has("observations_generator")) {
      const Config& og = cfg["observations_generator"];
      for (size_t i = 0; i < og.size(); i++) {
        const std::string cn = class_of(og.at(i));
        if (ends_with(cn, "::Generator") || cn == "Generator") continue;  // point clouds into 'raw': what onLidar* does
        if (!ends_with(cn, "GeneratorEdgesFromRangeImage")) unsupported("observations_generator " + cn);
        if (depth_input) unsupported("two GeneratorEdgesFromRangeImage entries");
        if (og.size() != 1) unsupported("GeneratorEdgesFromRangeImage beside another generator");
        if (timestamp_method != MH_TS_NONE) unsupported("FilterAdjustTimestamps with a depth-image generator (there is no 'raw')");
        const Config& p = og.at(i)["params"];
        steps.emplace_back();
        Step& st = steps.back();
        st.kind = Kind::EdgesFromRangeImage;
        st.pass = 0;
        st.cls = cn;
        st.out = {p.getOr("target_layer", "edges"), p.getOr("planes_target_layer", "planes")};
        if (st.out[0].empty() || st.out[1].empty() || st.out[0] == st.out[1] || st.out[0] == "raw" || st.out[1] == "raw")
          unsupported(cn + " needs two distinct layers target_layer and planes_target_layer");
        const double W = p.has("row_window_length") ? to_double(p["row_window_length"].asString()) : 6.0;
        if (!(W >= 1 && W <= 64) || W != std::floor(W)) unsupported(cn + " with row_window_length outside 1..64");
        st.row_window_length = (uint32_t)W;
        st.score_threshold = 10.0;
        if (p.has("score_threshold")) parameterFromConfig(p, "score_threshold", &st.score_threshold, false);
        depth_input = true;
        known = {st.out[0], st.out[1]};
      }
    }
    if (cfg.has("observations_filter_1st_pass")) load_pass(cfg["observations_filter_1st_pass"], 1, known);
    if (cfg.has("observations_filter_2nd_pass")) load_pass(cfg["observations_filter_2nd_pass"], 2, known);
    for (const auto& st : steps) has_2nd_pass = has_2nd_pass || st.pass == 2;
    const Config& gen = cfg["localmap_generator"];
    for (size_t i = 0; i < gen.size(); i++) {
      const Config& p = gen.at(i)["params"];
      MapSlot m;
      m.name = p.getOr("target_layer", "localmap");
      m.def = p["metric_map_definition"];
      const std::string c = m.def["class"].asString();
      if (!ends_with(c, "HashedVoxelPointCloud") && !ends_with(c, "NDT") && !ends_with(c, "CVoxelMap") &&
          !ends_with(c, "SparseTreesPointCloud"))
        unsupported("local map class '" + c + "' (HashedVoxelPointCloud, NDT, CVoxelMap, SparseTreesPointCloud)");
      for (const auto& o : maps)
        if (o.name == m.name) unsupported("two local maps named '" + m.name + "'");
      maps.push_back(m);
    }
    if (maps.empty()) unsupported("localmap_generator is empty");
    const Config& mg = cfg["insert_observation_into_local_map"];
    for (size_t i = 0; i < mg.size(); i++) {
      if (!ends_with(class_of(mg.at(i)), "FilterMerge")) unsupported("insert_observation_into_local_map: " + class_of(mg.at(i)));
      const Config& mp = mg.at(i)["params"];
      const std::string layer = mp["input_pointcloud_layer"].asString(), target = mp.getOr("target_layer", "localmap");
      if (!known.count(layer)) unsupported("FilterMerge reads layer '" + layer + "', which the filters do not leave");
      if (mp.has("input_layer_in_local_coordinates") && !to_bool(mp["input_layer_in_local_coordinates"].asString()))
        unsupported("FilterMerge with input_layer_in_local_coordinates: false");
      size_t k = 0;
      while (k < maps.size() && maps[k].name != target) k++;
      if (k == maps.size()) unsupported("FilterMerge into '" + target + "', which no localmap_generator entry defines");
      merges.emplace_back(layer, k);
    }
    if (merges.empty()) unsupported("insert_observation_into_local_map holds no FilterMerge");
  }
};

// ================================================================== driver
struct LidarOdometry::RawInput {
  size_t n = 0;
  const float *x = nullptr, *y = nullptr, *z = nullptr, *t = nullptr;  // channel arrays, or ...
  const void* data = nullptr;                                           // ... interleaved records
  size_t point_step = 0, off_x = 0, off_y = 0, off_z = 0;
  long long off_t = -1;
  long long off_i = -1;  // float32 intensity inside the record, or -1
  const uint16_t* depth = nullptr;  // ... or a range image of cam.rows x cam.cols (onDepthImage; n = its pixel count)
  mh_range_image_params cam{};
  // ... or the merged cloud of a rig's group, already in raw_ (onLidarFrom): its labels in merge order, the one that completed it
  const std::vector<std::string>* merged_labels = nullptr;
  const std::string* trigger_label = nullptr;
  bool same(const RawInput& o) const {
    return depth == o.depth && cam.rows == o.cam.rows && cam.cols == o.cam.cols && n == o.n && x == o.x && y == o.y && z == o.z && t == o.t && data == o.data && point_step == o.point_step &&
           off_x == o.off_x && off_y == o.off_y && off_z == o.off_z && off_t == o.off_t && off_i == o.off_i;
  }
};

struct LidarOdometry::Prefetch {
  RawInput req;  // announced, waiting for the current scan to reach its launch point
  RawInput in;   // handed to the worker
  bool requested = false, launched = false;
  int slot = 0;               // which of the two prefetch sets the worker fills / filled
  mh_preprocess_params pp{};  // the filter parameters the worker used
  // the worker: ONE thread that lives as long as the driver and takes a task per scan (a std::async per scan created a
  // thread per scan: ~20 us of the main thread's time right before its alignment)
  struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> task;
    bool has_task = false, busy = false, stop = false;
    std::exception_ptr error;
    void start() {
      th = std::thread([this] {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
          cv.wait(lk, [this] { return has_task || stop; });
          if (stop) return;
          std::function<void()> t = std::move(task);
          has_task = false;
          lk.unlock();
          std::exception_ptr e;
          try { t(); } catch (...) { e = std::current_exception(); }
          lk.lock();
          error = e;
          busy = false;
          cv.notify_all();
        }
      });
    }
    void submit(std::function<void()> t) {
      if (!th.joinable()) start();
      std::lock_guard<std::mutex> lk(m);
      task = std::move(t);
      has_task = busy = true;
      error = nullptr;
      cv.notify_all();
    }
    void wait() {  // rethrows what the task threw
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [this] { return !busy; });
      if (error) {
        std::exception_ptr e = error;
        error = nullptr;
        std::rethrow_exception(e);
      }
    }
    ~Worker() {
      if (th.joinable()) {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        th.join();
      }
    }
  } worker;
  bool on_worker = false;
  void join() {
    if (on_worker) {
      on_worker = false;
      worker.wait();
    }
  }
};

LidarOdometry::LidarOdometry(std::shared_ptr<DeviceContext> ctx) : ctx_(std::move(ctx)), pf_(new Prefetch) {}
LidarOdometry::~LidarOdometry() {
  cancel_prefetch();
  if (batcher_) batcher_->forgetOwner(this);
  if (params_.simplemap.generate && !params_.simplemap.save_final_map_to_file.empty()) {  // (:1884-1903: "at destruction time")
    try {
      saveKeyFrames(params_.simplemap.save_final_map_to_file);
    } catch (const std::exception& e) {
      fprintf(stderr, "[molahip] warning: the key-frames were not saved: %s\n", e.what());
    }
  }
}

// the relocalization: block (this implementation's own key): the pose-candidate search and the place descriptor
LidarOdometry::RelocalizationOptions relocalization_options(const Config& cfg) {
  LidarOdometry::RelocalizationOptions o;
  if (cfg.has("relocalization")) {
    const Config& r = cfg["relocalization"];
    if (r.has("score_threshold") && !r["score_threshold"].isNull()) o.score_threshold = r["score_threshold"].asString();
    if (r.has("step_xy") && !r["step_xy"].isNull()) o.step_xy = to_double(r["step_xy"].asString());
    if (r.has("step_yaw_deg")) o.step_yaw_deg = to_double(r["step_yaw_deg"].asString());
    if (r.has("sigmas")) o.sigmas = to_double(r["sigmas"].asString());
    if (r.has("refine_top_k")) o.refine_top_k = (uint32_t)to_double(r["refine_top_k"].asString());
    if (r.has("max_candidates")) o.max_candidates = (uint32_t)to_double(r["max_candidates"].asString());
    auto num = [&](const char* k, double& v) { if (r.has(k)) v = to_double(r[k].asString()); };
    auto cnt = [&](const char* k, uint32_t& v) { if (r.has(k)) v = (uint32_t)to_double(r[k].asString()); };
    cnt("place_rings", o.place_rings);
    cnt("place_sectors", o.place_sectors);
    num("place_min_range", o.place_min_range);
    num("place_max_range", o.place_max_range);
    num("place_z_min", o.place_z_min);
    num("place_z_max", o.place_z_max);
    cnt("place_top_k", o.place_top_k);
    num("place_sigma_xy", o.place_sigma_xy);
    num("place_sigma_yaw_deg", o.place_sigma_yaw_deg);
    if (o.place_rings < 1 || o.place_rings > MH_PLACE_MAX_RINGS || o.place_sectors < 8 || o.place_sectors > MH_PLACE_MAX_SECTORS || o.place_sectors % 8 ||
        !(o.place_min_range >= 0.0) || !(o.place_min_range < o.place_max_range) || !std::isfinite(o.place_max_range) || !(o.place_z_min < o.place_z_max) ||
        !std::isfinite(o.place_z_min) || !std::isfinite(o.place_z_max) || o.place_top_k < 1 || !(o.place_sigma_xy >= 0.0) || !std::isfinite(o.place_sigma_xy) ||
        !(o.place_sigma_yaw_deg >= 0.0) || !std::isfinite(o.place_sigma_yaw_deg))
      throw std::runtime_error("LidarOdometry (HIP): relocalization: place_rings in [1, 32], place_sectors a multiple of 8 in [8, 128], 0 <= place_min_range "
                               "< place_max_range, place_z_min < place_z_max, place_top_k >= 1, place_sigma_xy >= 0 and place_sigma_yaw_deg >= 0 are required");
    if (!(o.step_xy >= 0.0) || !(o.step_yaw_deg > 0.0) || !(o.sigmas > 0.0) || o.refine_top_k < 1 ||
        o.max_candidates < 1 || o.max_candidates > MH_SCORE_MAX_POSES)
      throw std::runtime_error("LidarOdometry (HIP): relocalization: step_xy >= 0, step_yaw_deg > 0, sigmas > 0, refine_top_k >= 1 and "
                               "1 <= max_candidates <= " + std::to_string(MH_SCORE_MAX_POSES) + " are required");
  }
  return o;
}

// the lost_recovery: block (this implementation's own key)
LostRecoveryOptions LostRecoveryOptions::FromConfig(const Config& cfg) {
  LostRecoveryOptions o;
  if (cfg.has("lost_recovery") && !cfg["lost_recovery"].isNull()) {
    const Config& c = cfg["lost_recovery"];
    auto given = [&](const char* k) { return c.has(k) && !c[k].isNull(); };
    if (given("enabled")) {
      const std::string s = c["enabled"].asString();
      if (s == "true" || s == "True" || s == "1" || s == "yes") o.enabled = true;
      else if (s == "false" || s == "False" || s == "0" || s == "no") o.enabled = false;
      else throw std::runtime_error("lost_recovery: enabled must be true or false");
    }
    auto cnt = [&](const char* k, uint32_t& v, double lo) {
      if (!given(k)) return;
      const std::string s = c[k].asString();
      char* end = nullptr;
      const double d = strtod(s.c_str(), &end);
      if (end == s.c_str() || *end != 0 || !(d >= lo) || !(d <= 4294967295.0) || d != std::floor(d))
        throw std::runtime_error(std::string("lost_recovery: ") + k + " must be an integer >= " + std::to_string((int)lo));
      v = (uint32_t)d;
    };
    auto num = [&](const char* k, double& v) {
      if (!given(k)) return;
      const std::string s = c[k].asString();
      char* end = nullptr;
      v = strtod(s.c_str(), &end);
      if (end == s.c_str() || *end != 0) v = NAN;  // (refused by validate())
    };
    cnt("bad_scans_to_lost", o.bad_scans_to_lost, 1.0);
    if (given("method")) o.method = c["method"].asString();
    num("near_sigma_xy", o.near_sigma_xy);
    num("near_sigma_yaw_deg", o.near_sigma_yaw_deg);
    cnt("retry_every_n_scans", o.retry_every_n_scans, 1.0);
    cnt("max_attempts", o.max_attempts, 0.0);
  }
  o.validate();
  return o;
}

void LostRecoveryOptions::validate() const {
  if (bad_scans_to_lost < 1) throw std::runtime_error("lost_recovery: bad_scans_to_lost must be an integer >= 1");
  if (method != "near" && method != "keyframes" && method != "near_then_keyframes")
    throw std::runtime_error("lost_recovery: method must be one of near, keyframes, near_then_keyframes; it is '" + method + "'");
  if (!(near_sigma_xy >= 0.0) || !std::isfinite(near_sigma_xy)) throw std::runtime_error("lost_recovery: near_sigma_xy must be finite and >= 0");
  if (!(near_sigma_yaw_deg >= 0.0) || !std::isfinite(near_sigma_yaw_deg))
    throw std::runtime_error("lost_recovery: near_sigma_yaw_deg must be finite and >= 0");
  if (retry_every_n_scans < 1) throw std::runtime_error("lost_recovery: retry_every_n_scans must be an integer >= 1");
}

// ---- LostRecovery: the rule is in LidarOdometry.h
bool LostRecovery::served(bool succeeded, Fields& f) {
  const uint32_t own = own_pending_;
  own_pending_ = 0;
  if (own) {
    f.recovery_attempt = own;
    attempts_++;
    attempts_this_loss_++;
  }
  if (succeeded) {
    f.recovery_succeeded = own != 0;
    if (lost_) {
      lost_ = false;
      times_recovered_++;
    }
    bad_streak_ = good_streak_ = 0;
    return false;
  }
  if (own) wait_ = o_.retry_every_n_scans;
  return own != 0;
}

void LostRecovery::gate(bool icp_good, Fields& f) {
  if (icp_good) {
    bad_streak_ = 0;
    if (lost_ && ++good_streak_ >= o_.bad_scans_to_lost) {
      lost_ = false;
      good_streak_ = 0;
      times_recovered_++;
    }
  } else {
    bad_streak_++;
    good_streak_ = 0;
    if (!lost_ && bad_streak_ >= o_.bad_scans_to_lost) {
      lost_ = true;
      times_lost_++;
      attempts_this_loss_ = 0;
      near_done_ = false;
      wait_ = 0;
    }
  }
  f.bad_streak = bad_streak_;
}

uint32_t LostRecovery::due(bool request_pending, bool near_fits) {
  if (!lost_) return 0;
  if (wait_ > 0) wait_--;
  if (request_pending || wait_ > 0 || gaveUp()) return 0;
  const bool near = o_.method == "near" || (o_.method == "near_then_keyframes" && !near_done_);
  if (!near) return 2;
  near_done_ = true;
  if (near_fits) return 1;
  skipped_++;  // no request, no device work: not an attempt
  if (o_.method == "near_then_keyframes") return 2;
  wait_ = o_.retry_every_n_scans;
  return 0;
}

namespace {
// lost_recovery: with an AlignBatcher, whichever of initialize() and setAlignBatcher() comes second: relocalizeInKeyFrames' refusal
const char* const kNoRecoveryWithBatcher = "enabled: LidarOdometry::relocalizeInKeyFrames: not available with an AlignBatcher (the batch protocol has "
                                           "no slot for the extra alignments of one member)";
// online_map_cleaning: likewise
const char* const kNoLiveCleaningWithBatcher = "enabled is not available with an AlignBatcher (the instances of a lock-step batch share one "
                                               "round of alignments; map updates queued between them are not part of its protocol)";
// gyro_deskew: likewise
const char* const kNoGyroDeskewWithBatcher = "enabled is not available with an AlignBatcher (a lock-step batch prepares its members' scans with "
                                             "mh_scan_preprocess_batch and the constant twist; it has no slot for a motion table per member)";
}  // namespace

void LidarOdometry::initialize(const Config& cfg) {
  if (plan_ || gplan_) throw std::runtime_error("LidarOdometry::initialize() called twice; create a new object instead");
  params_.load_from(cfg["params"]);
  params_.attachToParameterSource(source_);
  if (cfg.has("navstate_fuse_params")) navstate_.initialize(cfg["navstate_fuse_params"]);
  // the default chain first (its fused path, prefetch and batching); any other chain of implemented filters as a general plan
  try {
    if (GeneralPlan::wants_depth_input(cfg))  // (the default chain reads 'raw': a depth-image file always takes the general plan)
      throw std::runtime_error("unsupported observation filter chain: depth-image generator");
    auto plan = std::make_unique<FilterPlan>();
    plan->load(cfg);
    plan_ = std::move(plan);
    plan_->attachToParameterSource(source_);
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).find("unsupported observation filter chain") == std::string::npos) throw;
    auto g = std::make_unique<GeneralPlan>();
    g->intensity_input = intensity_input_;
    g->load(cfg);  // throws its own "unsupported observation filter chain" naming what is implemented
    gplan_ = std::move(g);
    gplan_->attachToParameterSource(source_);
  }

  if (params_.lidar_count < 1 || params_.lidar_count > MH_MAX_MERGE_SOURCES)
    throw std::runtime_error("LidarOdometry (HIP): params.multiple_lidars.lidar_count is " + std::to_string(params_.lidar_count) +
                             "; the device merges 1.." + std::to_string(MH_MAX_MERGE_SOURCES) + " sensors (MH_MAX_MERGE_SOURCES)");
  if (params_.lidar_count > 1 && gplan_ && gplan_->depth_input)
    throw std::runtime_error("LidarOdometry (HIP): params.multiple_lidars.lidar_count > 1 on a depth-image pipeline: rigs of depth "
                             "cameras are not implemented (one camera carries its pose in onDepthImage)");
  sync_ = SensorSync(params_.lidar_count, params_.max_time_offset);
  label_patterns_.clear();
  for (const auto& re : params_.lidar_sensor_labels) {
    try {
      label_patterns_.emplace_back(re);
    } catch (const std::regex_error& e) {
      throw std::runtime_error("LidarOdometry (HIP): params.lidar_sensor_labels: '" + re + "' is not a regular expression: " + e.what());
    }
  }

  // ICP pipelines (:340-358)
  auto t0 = icp_pipeline_from_yaml(cfg["icp_settings_with_vel"], ctx_);
  icp_[0] = std::get<0>(t0);
  icp_params_[0] = std::get<1>(t0);
  if (cfg.has("icp_settings_without_vel")) {
    auto t1 = icp_pipeline_from_yaml(cfg["icp_settings_without_vel"], ctx_);
    icp_[1] = std::get<0>(t1);
    icp_params_[1] = std::get<1>(t1);
  } else {
    icp_[1] = icp_[0];
    icp_params_[1] = icp_params_[0];
  }
  for (auto& icp : icp_) {
    icp->attachToParameterSource(source_);
    icp->setKeepFinalPairings(false);
    icp->fuseGatedMatchers(true);  // gated blocks (lidar3d-near-far.yaml:183) on the device loop; MOLA_HIP_FUSE_GATES=0: as before
    icp->fuseMultiPairings(true);  // pairingsPerPoint > 1 likewise (profiles/layers_kbest.md); MOLA_HIP_FUSE_KBEST=0: as before
    icp->fusePlaneMatchers(true);  // Matcher_Point2Plane on point layers likewise (profiles/layers_planes.md); MOLA_HIP_FUSE_PLANES=0: as before
  }
  // local map definition (yaml:213-242), instantiated at the first key-frame when its $f{} formulas can be evaluated
  const Config& gen = cfg["localmap_generator"];
  if (gen.size() < 1) throw std::runtime_error("localmap_generator is empty");
  map_def_ = gen.at(0)["params"]["metric_map_definition"];

  // initial_localization (yaml:147-151) and this implementation's relocalization: block
  init_loc_ = InitialLocalization();
  if (cfg.has("initial_localization")) {
    const Config& il = cfg["initial_localization"];
    if (il.has("enabled")) init_loc_.enabled = to_bool(il["enabled"].asString());
    if (il.has("method")) init_loc_.method = il["method"].asString();
    if (!ends_with(init_loc_.method, "FixedPose"))
      throw std::runtime_error("LidarOdometry (HIP): initial_localization.method '" + init_loc_.method +
                               "' is not implemented: only InitLocalization::FixedPose is (there are no GNSS inputs here)");
    if (il.has("fixed_initial_pose")) {
      const Config& fp = il["fixed_initial_pose"];
      if (fp.size() != 6) throw std::runtime_error("LidarOdometry (HIP): initial_localization.fixed_initial_pose needs 6 values (x y z yaw pitch roll)");
      double v[6];
      for (size_t i = 0; i < 6; i++) v[i] = to_double(fp.at(i).asString());
      init_loc_.fixed_initial_pose = TPose3D{v[0], v[1], v[2], v[3], v[4], v[5]};
    }
    if (il.has("relocalize_sigmas") && il["relocalize_sigmas"].size() > 0) {
      const Config& rs = il["relocalize_sigmas"];
      if (rs.size() != 3) throw std::runtime_error("LidarOdometry (HIP): initial_localization.relocalize_sigmas needs 3 values (sigma_x [m], sigma_y [m], sigma_yaw [deg])");
      for (size_t i = 0; i < 3; i++) {
        init_loc_.relocalize_sigmas[i] = to_double(rs.at(i).asString());
        if (!(init_loc_.relocalize_sigmas[i] >= 0.0) || !std::isfinite(init_loc_.relocalize_sigmas[i]))
          throw std::runtime_error("LidarOdometry (HIP): initial_localization.relocalize_sigmas must be finite and >= 0");
      }
      init_loc_.relocalize = true;
    }
  }
  reloc_opts_ = relocalization_options(cfg);

  // a saved map (:465-470): read now, names held against the plan's; the device maps are made by reset()
  loaded_maps_.clear();
  if (!params_.load_existing_local_map.empty()) {
    const std::string& path = params_.load_existing_local_map;
    loaded_maps_ = molahip_host::read_local_map_file(path);
    std::vector<std::string> want;
    if (gplan_) for (const auto& m : gplan_->maps) want.push_back(m.name);
    else want.push_back(plan_->map_layer);
    std::vector<std::string> have;
    for (const auto& r : loaded_maps_) have.push_back(r.name);
    auto sorted = [](std::vector<std::string> v) { std::sort(v.begin(), v.end()); return v; };
    if (sorted(want) != sorted(have)) {
      auto join = [](const std::vector<std::string>& v) { std::string o; for (const auto& x : v) o += (o.empty() ? "'" : ", '") + x + "'"; return o; };
      throw std::runtime_error("LidarOdometry (HIP): params.local_map_updates.load_existing_local_map: local map file '" + path + "' holds the maps " +
                               join(have) + ", the pipeline's localmap_generator makes " + join(want) + ": the names must match");
    }
  }

  // key-frames of the session (params.simplemap)
  if (params_.simplemap.generate_lazy_load_scan_files)
    throw std::runtime_error("LidarOdometry (HIP): params.simplemap.generate_lazy_load_scan_files: true is not implemented: a key-frame file "
                             "holds its layers itself (molahip_host/keyframe_file.h)");
  kf_store_ = KeyFrameStore(params_.simplemap.measure_from_last_kf_only);
  loaded_keyframes_ = molahip_host::KeyFrameSet();
  if (!params_.simplemap.load_existing_simple_map.empty()) {
    loaded_keyframes_ = molahip_host::read_keyframe_file(params_.simplemap.load_existing_simple_map);
    std::vector<std::string> want, have;
    if (gplan_) for (const auto& m : gplan_->maps) want.push_back(m.name);
    else want.push_back(plan_->map_layer);
    for (const auto& t : loaded_keyframes_.maps) have.push_back(t.name);
    if (want != have)
      throw std::runtime_error("LidarOdometry (HIP): params.simplemap.load_existing_simple_map: the key-frame file '" +
                               params_.simplemap.load_existing_simple_map + "' was recorded for other target maps than this pipeline's");
  }

  // online_loop_closure: (LoopClosure.h): read and checked whether enabled or not
  {
    const OnlineLoopClosureOptions ol = OnlineLoopClosureOptions::FromConfig(cfg);
    loop_enabled_ = ol.enabled;
    loop_correct_ = ol.correct_driver;
    loop_cfg_ = Config();
    if (loop_enabled_) {
      (void)LoopClosureOptions::FromConfig(cfg);  // (the closer's gates and weights: out of range is refused here, not at the first key-frame)
      if (!params_.simplemap.generate)
        throw std::runtime_error("LidarOdometry (HIP): online_loop_closure: enabled needs params.simplemap.generate: true: the loop closer "
                                 "works on the key-frame store");
      std::vector<std::string> names;
      auto refuse_occupancy = [](const std::string& name, const Config& def) {
        if (ends_with(def["class"].asString(), "CVoxelMap"))
          throw std::runtime_error("LidarOdometry (HIP): online_loop_closure: local map '" + name + "' is a 'CVoxelMap': an occupancy map cannot be "
                                   "built from key-frames, so no submap to verify a loop in and no map to rebuild after one (HashedVoxelPointCloud, "
                                   "NDT and SparseTreesPointCloud can)");
      };
      if (gplan_) {
        for (const auto& m : gplan_->maps) {
          refuse_occupancy(m.name, m.def);
          names.push_back(m.name);
        }
      } else {
        refuse_occupancy(plan_->map_layer, map_def_);
        names.push_back(plan_->map_layer);
      }
      check_loop_closure_icp(*icp_[1], names, "LidarOdometry (HIP): online_loop_closure");
      loop_cfg_ = cfg;
    }
  }

  // lost_recovery: (LidarOdometry.h): read and checked whether enabled or not; what it needs is asked for only when enabled
  {
    const LostRecoveryOptions lr = LostRecoveryOptions::FromConfig(cfg);
    if (lr.enabled) {
      const std::string who = "LidarOdometry (HIP): lost_recovery: ";
      if (lr.needsKeyFrames() && !params_.simplemap.generate && params_.simplemap.load_existing_simple_map.empty())
        throw std::runtime_error(who + "method '" + lr.method + "' needs key-frames to search: params.simplemap.generate: true or "
                                 "params.simplemap.load_existing_simple_map (method: near needs none)");
      if (loop_enabled_)
        throw std::runtime_error(who + "enabled together with online_loop_closure: enabled is not implemented (the raw chain of the loop "
                                 "closer has no rule for a jump of the pose)");
      if (batcher_) throw std::runtime_error(who + kNoRecoveryWithBatcher);  // (setAlignBatcher says the same when it comes second)
      try {  // (what the requests themselves refuse of the plan: an ICP block without a matcher to score with)
        std::string g, l;
        check_can_relocalize(lr.needsKeyFrames() ? "relocalizeInKeyFrames" : "relocalizeNearPose", g, l);
      } catch (const std::runtime_error& e) {
        throw std::runtime_error(who + "enabled, but " + e.what());
      }
    }
    lost_ = LostRecovery(lr);
  }

  // online_map_cleaning: (LiveMapCleaning.h): read and checked whether enabled or not
  {
    live_opts_ = OnlineMapCleaningOptions::FromConfig(cfg);
    live_cleaner_.reset();
    if (live_opts_.enabled) {
      const std::string who = "LidarOdometry (HIP): online_map_cleaning: ";
      std::vector<std::pair<std::string, bool>> maps;  // the plan's maps: name, is an occupancy map
      if (gplan_)
        for (const auto& m : gplan_->maps) maps.emplace_back(m.name, ends_with(m.def["class"].asString(), "CVoxelMap"));
      else
        maps.emplace_back(plan_->map_layer, ends_with(map_def_["class"].asString(), "CVoxelMap"));
      for (const auto& t : live_opts_.target_maps) {
        const auto it = std::find_if(maps.begin(), maps.end(), [&](const auto& m) { return m.first == t; });
        if (it == maps.end()) throw std::runtime_error(who + "target_maps names '" + t + "', which is no local map of this pipeline");
        if (it->second)
          throw std::runtime_error(who + "target map '" + t + "' is a 'CVoxelMap': an occupancy map stores no points to erase and is cleared by "
                                   "its own ray tracing (HashedVoxelPointCloud, NDT and SparseTreesPointCloud maps can be targets)");
      }
      if (live_opts_.target_maps.empty() && std::all_of(maps.begin(), maps.end(), [](const auto& m) { return m.second; }))
        throw std::runtime_error(who + "enabled, but every local map of this pipeline is a 'CVoxelMap': there is no point map to erase from");
      if (!live_opts_.view_layer.empty()) {
        bool known = false;
        if (gplan_) {
          known = live_opts_.view_layer == "raw";
          for (const auto& st : gplan_->steps)
            known = known || std::find(st.out.begin(), st.out.end(), live_opts_.view_layer) != st.out.end();
        } else {
          known = live_opts_.view_layer == plan_->layer_for_map || live_opts_.view_layer == plan_->layer_for_icp;
        }
        if (!known) throw std::runtime_error(who + "view_layer '" + live_opts_.view_layer + "' is no observation layer this pipeline's filters make");
      }
      if (loop_enabled_ && loop_correct_)
        throw std::runtime_error(who + "enabled together with online_loop_closure: correct_driver: true is not implemented (an accepted closure "
                                 "rebuilds the local maps from the key-frames, which would bring the erased points back)");
      if (batcher_) throw std::runtime_error(who + kNoLiveCleaningWithBatcher);  // (setAlignBatcher says the same when it comes second)
    }
  }

  // gyro_deskew: (GyroDeskew.h): read and checked whether enabled or not
  {
    gyro_opts_ = GyroDeskewOptions::FromConfig(cfg);
    gyro_buf_.setBufferSeconds(gyro_opts_.buffer_seconds);
    if (gyro_opts_.enabled) {
      const std::string who = "LidarOdometry (HIP): gyro_deskew: ";
      if (gplan_ && gplan_->depth_input)
        throw std::runtime_error(who + "enabled on a depth-image pipeline (GeneratorEdgesFromRangeImage): its pixels carry no time stamps, "
                                 "there is nothing to de-skew by");
      if (batcher_) throw std::runtime_error(who + kNoGyroDeskewWithBatcher);  // (setAlignBatcher says the same when it comes second)
    }
  }

  reset();  // device objects are created at the first scan: a pipeline can be loaded and checked without a GPU (a saved map
            // is restored here, which needs one)
}

void LidarOdometry::restore_loaded_maps() {
  if (!ctx_) ctx_ = DeviceContext::Default();
  auto rec_of = [&](const std::string& name) -> const molahip_host::LocalMapRecord& {
    for (const auto& r : loaded_maps_)
      if (r.name == name) return r;
    throw std::runtime_error("local map file: no map called '" + name + "'");  // (initialize() has checked the names)
  };
  if (gplan_) {
    for (auto& m : gplan_->maps) {
      const auto& r = rec_of(m.name);
      m.map = mp2p_icp_hip::make_local_map(r, ctx_);
      m.voxel_size = (double)r.params.voxel_size;
      m.remove_far = r.remove_voxels_farther_than;
    }
    local_map_ = gplan_->maps[0].map;
    map_voxel_size_ = gplan_->maps[0].voxel_size;
  } else {
    const auto& r = rec_of(plan_->map_layer);
    local_map_ = mp2p_icp_hip::make_local_map(r, ctx_);
    map_voxel_size_ = (double)r.params.voxel_size;
    remove_voxels_farther_than_ = r.remove_voxels_farther_than;
  }
  map_points_cached_ = gplan_ ? maps_total(false) : local_map_->size();
  map_voxels_cached_ = gplan_ ? maps_total(true) : local_map_->voxelCount();
  map_known_nonempty_ = map_points_cached_ != 0;
}

void LidarOdometry::saveLocalMaps(const std::string& path) const {
  std::vector<molahip_host::LocalMapRecord> recs;
  if (gplan_) {
    for (const auto& m : gplan_->maps) {
      if (!m.map) throw std::runtime_error("LidarOdometry::saveLocalMaps: local map '" + m.name + "' does not exist yet (no key-frame so far)");
      recs.push_back(m.map->snapshot(m.name, m.remove_far));
    }
  } else {
    if (!plan_ || !local_map_) throw std::runtime_error("LidarOdometry::saveLocalMaps: the local map does not exist yet (no key-frame so far)");
    recs.push_back(local_map_->snapshot(plan_->map_layer, remove_voxels_farther_than_));
  }
  molahip_host::write_local_map_file(path, recs);
}

std::vector<molahip_host::KeyFrameTarget> LidarOdometry::keyframe_targets() const {
  std::vector<molahip_host::KeyFrameTarget> out;
  auto target = [](const std::string& name, const HashedVoxelPointCloud& m, float remove_far) {
    molahip_host::KeyFrameTarget t;
    t.name = name;
    t.class_name = m.className();
    t.params = m.params();
    t.remove_voxels_farther_than = remove_far;
    return t;
  };
  if (gplan_) {
    for (const auto& m : gplan_->maps) out.push_back(target(m.name, *m.map, m.remove_far));
  } else {
    out.push_back(target(plan_->map_layer, *local_map_, remove_voxels_farther_than_));
  }
  return out;
}

void LidarOdometry::saveKeyFrames(const std::string& path) const {
  if (!kf_store_.set().frames.empty() && kf_store_.set().maps.empty())
    throw std::runtime_error("LidarOdometry::saveKeyFrames: the target maps are not known yet");  // (cannot happen: the first stored scan makes them)
  molahip_host::write_keyframe_file(path, kf_store_.set());
}

// params.simplemap.load_existing_simple_map: the new frames are appended under the file's header, so build_session_maps builds
// them with the file's class and mh_map_params: these must be the running plan's.  (remove_voxels_farther_than is not held
// against the plan: it follows the first scan's range estimate, and a session map is built without far removal.)
void LidarOdometry::check_loaded_keyframe_targets(const std::vector<molahip_host::KeyFrameTarget>& plan) const {
  const auto& file = loaded_keyframes_.maps;
  for (size_t k = 0; k < file.size() && k < plan.size(); k++) {  // (initialize() has checked the names and their order)
    const mh_map_params &a = file[k].params, &b = plan[k].params;
    const bool same = file[k].class_name == plan[k].class_name && a.voxel_size == b.voxel_size && a.max_points_per_voxel == b.max_points_per_voxel &&
                      a.index_mode == b.index_mode && a.min_distance_between_points == b.min_distance_between_points &&
                      a.ndt_max_eigen_ratio == b.ndt_max_eigen_ratio && a.ndt_min_points == b.ndt_min_points &&
                      a.far_voxel_metric == b.far_voxel_metric;
    if (!same)
      throw std::runtime_error("LidarOdometry (HIP): params.simplemap.load_existing_simple_map: the key-frame file '" +
                               params_.simplemap.load_existing_simple_map + "' was recorded for a map '" + file[k].name + "' of class " +
                               file[k].class_name + ", voxel size " + std::to_string(a.voxel_size) + ", cap " + std::to_string(a.max_points_per_voxel) +
                               "; this pipeline makes a " + plan[k].class_name + ", voxel size " + std::to_string(b.voxel_size) + ", cap " +
                               std::to_string(b.max_points_per_voxel) + ": class and map parameters must match for the session to be continued");
  }
}

// params.simplemap.generate: the decision of :1117-1138 (KeyFrameStore::decide) and, for a stored scan, its host copy -- pose,
// covariance, the twist of its last de-skew and, for a key-frame, the input layer of every FilterMerge step as the last run of
// the second pass left it (one blocking download on this instance's stream, after the scan's registration).
void LidarOdometry::store_keyframe(ScanRecord& rec, bool first_scan, bool icp_good, const double* cov) {
  const KeyFrameStore::Verdict v = kf_store_.decide(first_scan, icp_good, last_lidar_pose_, params_.simplemap.min_translation_between_keyframes,
                                                    params_.simplemap.min_rotation_between_keyframes, params_.simplemap.add_non_keyframes_too);
  if (!v.stored) return;
  StageTimer tt(profile_, "onLidar.5.store_keyframe");
  molahip_host::KeyFrame f;
  f.timestamp = rec.timestamp;
  std::copy(last_lidar_pose_.T, last_lidar_pose_.T + 12, f.pose);
  if (cov) std::copy(cov, cov + 36, f.cov);
  f.has_twist = rec.had_motion_model || rec.twist_corrections > 0;
  if (f.has_twist) {
    const double tw[6] = {rec.twist.vx, rec.twist.vy, rec.twist.vz, rec.twist.wx, rec.twist.wy, rec.twist.wz};
    std::copy(tw, tw + 6, f.twist);
  }
  f.has_points = v.keyframe;
  if (v.keyframe) {
    if (gplan_) {
      for (const auto& [name, k] : gplan_->merges) {
        molahip_host::KeyFrameLayer l;
        l.map_index = (uint32_t)k;
        if (gplan_->alive.count(name))  // (a layer the filters did not leave this scan: an empty entry, as nothing is merged)
          (name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name))->download(l.x, l.y, l.z);
        f.layers.push_back(std::move(l));
      }
    } else {
      molahip_host::KeyFrameLayer l;
      for_map_->download(l.x, l.y, l.z);
      f.layers.push_back(std::move(l));
    }
  }
  kf_store_.add(std::move(f));
  rec.simplemap_frame = true;
  rec.simplemap_keyframe = v.keyframe;
}

void LidarOdometry::seed_motion_model(double t, const CPose3D& pose) {  // "fake an evolution to have an initial velocity estimation" (:784-790)
  navstate_.fuse_pose(t - 0.2, pose);  // (cov null: the 1e-12 diagonal of :783)
  navstate_.fuse_pose(t - 0.1, pose);
}

void LidarOdometry::scan_layers(mp2p_icp_hip::metric_map_t& obs, mp2p_icp_hip::metric_map_t& glob) const {
  if (gplan_) {  // every layer the filters leave, every map (the ICP pipeline's matchers pick their pairs)
    for (const auto& name : gplan_->alive)
      obs.layers[name] = name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name);
    for (const auto& m : gplan_->maps)
      if (m.map) glob.layers[m.name] = m.map;
  } else {
    obs.layers[plan_->layer_for_icp] = for_icp_;
    obs.layers[plan_->layer_for_map] = for_map_;
    glob.layers[plan_->map_layer] = local_map_;
  }
}

// ================================================================== relocalization
namespace {
void relocalization_grid_nodes(const double cov[36], double step_xy, double step_yaw_rad, double sigmas, size_t& nx, size_t& ny, size_t& nyaw) {
  if (!(step_xy > 0.0) || !(step_yaw_rad > 0.0) || !(sigmas > 0.0) || !std::isfinite(step_xy) || !std::isfinite(step_yaw_rad) || !std::isfinite(sigmas))
    throw std::runtime_error("relocalization_grid: the steps and sigmas must be finite and > 0");
  auto nodes = [&](double var, double step) -> size_t {
    if (!(var >= 0.0) || !std::isfinite(var)) throw std::runtime_error("relocalization_grid: the covariance diagonal must be finite and >= 0");
    const double half = std::ceil(sigmas * std::sqrt(var) / step);
    if (!(half < 1.0e7)) throw std::runtime_error("relocalization_grid: more than max_candidates candidates: coarsen the steps");
    return 2 * (size_t)half + 1;
  };
  nx = nodes(cov[0], step_xy), ny = nodes(cov[7], step_xy), nyaw = nodes(cov[21], step_yaw_rad);
}
}  // namespace

bool relocalization_grid_fits(const double cov[36], double step_xy, double step_yaw_rad, double sigmas, size_t max_candidates) {
  size_t nx, ny, nyaw;
  relocalization_grid_nodes(cov, step_xy, step_yaw_rad, sigmas, nx, ny, nyaw);
  return !(nx * ny > max_candidates || nx * ny * nyaw > max_candidates);
}

std::vector<TPose3D> relocalization_grid(const TPose3D& mean, const double cov[36], double step_xy, double step_yaw_rad, double sigmas,
                                         size_t max_candidates) {
  size_t nx, ny, nyaw;
  relocalization_grid_nodes(cov, step_xy, step_yaw_rad, sigmas, nx, ny, nyaw);
  if (nx * ny > max_candidates || nx * ny * nyaw > max_candidates)
    throw std::runtime_error("relocalization_grid: " + std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nyaw) +
                             " candidates exceed max_candidates (" + std::to_string(max_candidates) + "): coarsen the steps or tighten the covariance");
  std::vector<TPose3D> out;
  out.reserve(nx * ny * nyaw);
  auto off = [](size_t i, size_t n, double step) { return ((double)i - (double)(n - 1) / 2.0) * step; };
  for (size_t ix = 0; ix < nx; ix++)
    for (size_t iy = 0; iy < ny; iy++)
      for (size_t iw = 0; iw < nyaw; iw++) {
        TPose3D p = mean;
        p.x = mean.x + off(ix, nx, step_xy);
        p.y = mean.y + off(iy, ny, step_xy);
        p.yaw = mean.yaw + off(iw, nyaw, step_yaw_rad);
        out.push_back(p);
      }
  return out;
}

namespace {
// the (global, local) layers a relocalization scores: the first pointLayerMatches entry of the first enabled
// Matcher_Points_DistanceThreshold of an ICP block
bool scored_layers(ICP& icp, std::string& global, std::string& local) {
  for (const auto& m : icp.matchers()) {
    auto* pm = dynamic_cast<mp2p_icp_hip::Matcher_Points_DistanceThreshold*>(m.get());
    if (!pm || !pm->enabled || pm->pointLayerMatches.empty()) continue;
    global = pm->pointLayerMatches[0].global;
    local = pm->pointLayerMatches[0].local;
    return true;
  }
  return false;
}
}  // namespace

double LidarOdometry::reloc_score_threshold(const std::string& global_layer) const {
  if (!reloc_opts_.score_threshold.empty()) return eval_now(reloc_opts_.score_threshold, source_.getVariableValues());
  std::shared_ptr<HashedVoxelPointCloud> g;
  if (gplan_) {
    for (const auto& m : gplan_->maps)
      if (m.name == global_layer) g = m.map;
  } else if (plan_ && plan_->map_layer == global_layer) {
    g = local_map_;
  }
  if (!g) return NAN;
  mh_map_info mi{};
  check(mh_map_get_info(g->handle(), &mi), "mh_map_get_info");
  return 0.5 * (double)mi.voxel_size;
}

void LidarOdometry::check_can_relocalize(const char* who, std::string& g, std::string& l, const CPose3D* mean) const {
  if (batcher_)
    throw std::runtime_error(std::string("LidarOdometry::") + who + ": not available with an AlignBatcher (the batch protocol has no slot for "
                             "the extra alignments of one member)");
  if (mean)
    for (int i = 0; i < 12; i++)
      if (!std::isfinite(mean->T[i])) throw std::runtime_error(std::string("LidarOdometry::") + who + ": non-finite pose");
  if (!scored_layers(*icp_[1], g, l))
    throw std::runtime_error(std::string("LidarOdometry::") + who + ": the no-motion-model ICP block has no enabled Matcher_Points_DistanceThreshold "
                             "to score candidates with");
}

void LidarOdometry::relocalizeNearPose(const CPose3D& mean, const double cov[36]) {
  if (!plan_ && !gplan_) throw std::runtime_error("LidarOdometry::relocalizeNearPose called before initialize()");
  std::string g, l;
  check_can_relocalize("relocalizeNearPose", g, l, &mean);
  // the candidate count is checked now, so that the caller can coarsen (when the defaults need a map that is not there yet: at
  // the scan that serves the request)
  const double thr = reloc_score_threshold(g);
  if (std::isfinite(thr)) {
    const double step = reloc_opts_.step_xy > 0 ? reloc_opts_.step_xy : thr;
    (void)relocalization_grid(mean.asTPose(), cov, step, reloc_opts_.step_yaw_deg * kDeg2Rad, reloc_opts_.sigmas, reloc_opts_.max_candidates);
  }
  RelocRequest rq;
  rq.mean = mean;
  for (int i = 0; i < 36; i++) rq.cov[i] = cov[i];
  reloc_request_ = rq;
  lost_.callerRequested();  // (place_recovery_request() says afterwards when the request is the driver's own)
}

void LidarOdometry::relocalizeInKeyFrames() {
  if (!plan_ && !gplan_) throw std::runtime_error("LidarOdometry::relocalizeInKeyFrames called before initialize()");
  std::string g, l;
  check_can_relocalize("relocalizeInKeyFrames", g, l);
  RelocRequest rq;
  for (int i = 0; i < 36; i++) rq.cov[i] = 0.0;
  rq.in_keyframes = true;
  reloc_request_ = rq;
  lost_.callerRequested();
}

// lost_recovery: the covariance of a `near` attempt, and whether its grid stays within relocalization.max_candidates (where
// relocalizeNearPose would throw; true while the searched map, whose voxel size the default step is, does not exist)
void LidarOdometry::near_attempt_cov(double cov[36]) const {
  const LostRecoveryOptions& o = lost_.options();
  std::fill(cov, cov + 36, 0.0);
  cov[0] = cov[7] = o.near_sigma_xy * o.near_sigma_xy;
  const double syaw = o.near_sigma_yaw_deg * kDeg2Rad;
  cov[21] = syaw * syaw;
}

bool LidarOdometry::near_attempt_fits() const {
  std::string g, l;
  if (!scored_layers(*icp_[1], g, l)) return true;
  const double thr = reloc_score_threshold(g);
  if (!std::isfinite(thr)) return true;
  double cov[36];
  near_attempt_cov(cov);
  return relocalization_grid_fits(cov, reloc_opts_.step_xy > 0 ? reloc_opts_.step_xy : thr, reloc_opts_.step_yaw_deg * kDeg2Rad, reloc_opts_.sigmas,
                                  reloc_opts_.max_candidates);
}

// lost_recovery: the driver's own request, made as a caller makes it
void LidarOdometry::place_recovery_request(uint32_t kind) {
  if (kind == 1) {
    double cov[36];
    near_attempt_cov(cov);
    relocalizeNearPose(lost_pose_, cov);
  } else {
    relocalizeInKeyFrames();
  }
  lost_.placed(kind);
}

std::vector<TPose3D> LidarOdometry::place_candidates(ScanRecord& rec, double step) {
  const RelocalizationOptions& o = reloc_opts_;
  const molahip_host::KeyFrameSet& set = kf_store_.set();
  // ---- 1. the index follows the store
  if (!place_index_) {
    mh_place_params pp{};
    pp.n_rings = o.place_rings;
    pp.n_sectors = o.place_sectors;
    pp.min_range = (float)o.place_min_range;
    pp.max_range = (float)o.place_max_range;
    pp.z_min = (float)o.place_z_min;
    pp.z_max = (float)o.place_z_max;
    place_index_ = std::make_unique<PlaceIndex>(pp, ctx_);
    place_frames_seen_ = 0;
  }
  if (place_frames_seen_ < set.frames.size()) {
    place_index_->addKeyFrames(set, place_frames_seen_);
    place_frames_seen_ = set.frames.size();
  }
  if (place_index_->size() == 0)
    throw std::runtime_error("LidarOdometry: relocalizeInKeyFrames: the key-frame store holds no frame with points: name the key-frame file of the "
                             "session in params.simplemap.load_existing_simple_map (MOLA_LOAD_SM)");
  std::shared_ptr<DevicePointCloud> layer;
  if (gplan_) {
    if (!gplan_->merges.empty()) {
      const std::string& name = gplan_->merges.front().first;
      if (gplan_->alive.count(name)) layer = name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name);
    }
  } else {
    layer = for_map_;
  }
  if (!layer) throw std::runtime_error("LidarOdometry: relocalizeInKeyFrames: the input layer of the first FilterMerge step is not among this scan's");
  // ---- 2. search, keep place_top_k
  std::vector<PlaceIndex::Match> m = place_index_->query(*layer);
  m.resize(std::min<size_t>(m.size(), o.place_top_k));
  rec.place_tried = true;
  // ---- 3. a grid around every kept frame, concatenated in rank order
  double cov[36] = {0};
  cov[0] = cov[7] = o.place_sigma_xy * o.place_sigma_xy;
  const double syaw = o.place_sigma_yaw_deg * kDeg2Rad;
  cov[21] = syaw * syaw;
  std::vector<TPose3D> cand;
  for (const PlaceIndex::Match& k : m) {
    rec.place_frames.push_back(k.frame);
    rec.place_shifts.push_back(k.shift);
    rec.place_dists.push_back(k.dist);
    CPose3D fp;
    std::copy(set.frames[k.frame].pose, set.frames[k.frame].pose + 12, fp.T);
    TPose3D rz;
    rz.yaw = -(double)k.shift * 2.0 * M_PI / (double)o.place_sectors;
    const CPose3D mean = fp + CPose3D(rz);
    const std::vector<TPose3D> g = relocalization_grid(mean.asTPose(), cov, step, o.step_yaw_deg * kDeg2Rad, o.sigmas, o.max_candidates);
    if (cand.size() + g.size() > o.max_candidates)
      throw std::runtime_error("relocalization_grid: " + std::to_string(cand.size() + g.size()) + " candidates over " + std::to_string(m.size()) +
                               " key-frames exceed max_candidates (" + std::to_string(o.max_candidates) + "): coarsen the steps or tighten the covariance");
    cand.insert(cand.end(), g.begin(), g.end());
  }
  return cand;
}

// ---- PlaceIndex
PlaceIndex::PlaceIndex(const mh_place_params& params, std::shared_ptr<DeviceContext> ctx) : ctx_(ctx ? std::move(ctx) : DeviceContext::Default()), params_(params) {
  check(mh_place_db_create(ctx_->get(), &params_, &db_), "mh_place_db_create");
}
PlaceIndex::~PlaceIndex() {
  if (db_) (void)mh_place_db_destroy(db_);
}
size_t PlaceIndex::addKeyFrames(const molahip_host::KeyFrameSet& set, size_t first) {
  std::vector<mh_map_frame> f;
  std::vector<uint32_t> idx;
  for (size_t k = first; k < set.frames.size(); k++) {
    const molahip_host::KeyFrame& kf = set.frames[k];
    if (!kf.has_points || kf.layers.empty() || kf.layers[0].x.empty()) continue;
    mh_map_frame e{};
    e.x = kf.layers[0].x.data(); e.y = kf.layers[0].y.data(); e.z = kf.layers[0].z.data();
    e.n = kf.layers[0].x.size();
    std::copy(kf.pose, kf.pose + 12, e.T);
    f.push_back(e);
    idx.push_back((uint32_t)k);
  }
  if (f.empty()) return 0;
  check(mh_place_db_add_frames(db_, f.data(), f.size(), MH_MEM_HOST), "mh_place_db_add_frames");
  frame_of_.insert(frame_of_.end(), idx.begin(), idx.end());
  return f.size();
}
std::vector<uint8_t> PlaceIndex::describe(const DevicePointCloud& layer) const {
  std::vector<uint8_t> d((size_t)params_.n_rings * params_.n_sectors);
  check(mh_place_describe(layer.handle(), &params_, d.data(), MH_MEM_HOST), "mh_place_describe");
  return d;
}
std::vector<PlaceIndex::Match> PlaceIndex::query(const DevicePointCloud& layer) const {
  const std::vector<uint8_t> q = describe(layer);
  std::vector<mh_place_match> out(frame_of_.size());
  check(mh_place_search(db_, q.data(), MH_MEM_HOST, out.data(), MH_MEM_HOST), "mh_place_search");
  std::vector<Match> m(out.size());
  for (size_t k = 0; k < out.size(); k++) m[k] = Match{frame_of_[k], out[k].shift, out[k].dist};
  std::stable_sort(m.begin(), m.end(), [](const Match& a, const Match& b) { return a.dist != b.dist ? a.dist < b.dist : a.frame < b.frame; });
  return m;
}

RelocalizationRefinement score_rank_refine(ICP& icp, const mp2p_icp_hip::Parameters& icp_params, const mp2p_icp_hip::metric_map_t& pcLocal,
                                           const mp2p_icp_hip::metric_map_t& pcGlobal, const std::string& global_layer, const std::string& local_layer,
                                           const std::vector<TPose3D>& cand, double score_threshold, uint32_t refine_top_k,
                                           std::map<std::string, double>* seconds) {
  const auto gi = pcGlobal.layers.find(global_layer);
  const auto li = pcLocal.layers.find(local_layer);
  auto global = gi == pcGlobal.layers.end() ? nullptr : std::dynamic_pointer_cast<HashedVoxelPointCloud>(gi->second);
  auto local = li == pcLocal.layers.end() ? nullptr : std::dynamic_pointer_cast<DevicePointCloud>(li->second);
  if (!global || !local)
    throw std::runtime_error("score_rank_refine: the layers '" + global_layer + "' / '" + local_layer + "' are not a device map and a device point layer of the maps given");
  RelocalizationRefinement out;
  const auto t0 = std::chrono::steady_clock::now();
  // ---- score: one launch over all candidates
  std::vector<double> poses(12 * cand.size());
  for (size_t c = 0; c < cand.size(); c++) {
    const CPose3D P(cand[c]);
    std::copy(P.T, P.T + 12, &poses[12 * c]);
  }
  std::vector<mh_pose_score> scores(cand.size());
  global->prepareSearch(score_threshold);
  check(mh_score_poses(global->handle(), local->handle(), poses.data(), cand.size(), score_threshold, 0.0, scores.data(), MH_MEM_HOST), "mh_score_poses");
  // ---- rank: (n_paired descending, cost ascending, index ascending)
  std::vector<uint32_t> order(cand.size());
  for (size_t c = 0; c < order.size(); c++) order[c] = (uint32_t)c;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (scores[a].n_paired != scores[b].n_paired) return scores[a].n_paired > scores[b].n_paired;
    return scores[a].cost < scores[b].cost;
  });
  order.resize(std::min<size_t>(order.size(), refine_top_k));
  out.ranks = order;
  for (uint32_t c : order) out.scores.push_back(scores[c]);
  const auto t1 = std::chrono::steady_clock::now();
  // ---- refine the kept candidates, one after another
  for (uint32_t c : order) {
    mp2p_icp_hip::Results res;
    icp.clearHooks();
    icp.align(pcLocal, pcGlobal, cand[c], icp_params, res, std::nullopt);
    if (!out.have || res.quality > out.best.quality) {  // (ties go to the better rank)
      out.best = res;
      out.have = true;
    }
  }
  if (seconds) {
    (*seconds)["score"] += std::chrono::duration<double>(t1 - t0).count();
    (*seconds)["refine"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  }
  return out;
}

void LidarOdometry::serve_relocalization(double t, ScanRecord& rec) {
  StageTimer tt(profile_, "onLidar.2.relocalize");
  const auto t_served = std::chrono::steady_clock::now();
  ICP& icp = *icp_[1];
  std::string gname, lname;
  if (!scored_layers(icp, gname, lname)) throw std::runtime_error("LidarOdometry: relocalization: no Matcher_Points_DistanceThreshold to score with");
  mp2p_icp_hip::metric_map_t obs, glob;
  scan_layers(obs, glob);
  const auto gi = glob.layers.find(gname);
  const auto li = obs.layers.find(lname);
  if (gi == glob.layers.end() || li == obs.layers.end() || !std::dynamic_pointer_cast<HashedVoxelPointCloud>(gi->second) ||
      !std::dynamic_pointer_cast<DevicePointCloud>(li->second))
    throw std::runtime_error("LidarOdometry: relocalization: the layers '" + gname + "' / '" + lname + "' of the no-motion-model ICP block are not among this scan's");
  const double thr = reloc_score_threshold(gname);
  const double step = reloc_opts_.step_xy > 0 ? reloc_opts_.step_xy : thr;
  // the candidate list: a grid around the given pose, or the grids around the key-frames the place search kept; everything
  // below is the same for both requests
  const std::vector<TPose3D> cand = reloc_request_->in_keyframes
                                        ? place_candidates(rec, step)
                                        : relocalization_grid(reloc_request_->mean.asTPose(), reloc_request_->cov, step,
                                                              reloc_opts_.step_yaw_deg * kDeg2Rad, reloc_opts_.sigmas, reloc_opts_.max_candidates);
  rec.relocalization_tried = true;
  rec.reloc_candidates = (uint32_t)cand.size();
  // ---- score, rank, refine (the step a loop closure's verification shares)
  const RelocalizationRefinement rr = score_rank_refine(icp, icp_params_[1], obs, glob, gname, lname, cand, thr, reloc_opts_.refine_top_k);
  rec.reloc_ranks = rr.ranks;
  rec.reloc_best_n_paired = rr.scores.empty() ? 0 : rr.scores[0].n_paired;
  profile_["relocalize.align_calls"] += (double)rr.ranks.size();
  const bool have = rr.have;
  const mp2p_icp_hip::Results& best = rr.best;
  rec.reloc_best_quality = have ? best.quality : 0.0;
  // ---- accept
  if (have && best.quality >= params_.min_icp_goodness) {
    navstate_.reset();
    seed_motion_model(t, best.optimal_tf.mean);
    last_lidar_pose_ = best.optimal_tf.mean;
    reloc_request_.reset();
    rec.relocalized = true;
  }
  if (lost_.options().enabled) note_served(rec, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_served).count());
}

// lost_recovery: the driver's own request is an attempt, and does not stay pending when it fails
void LidarOdometry::note_served(ScanRecord& rec, double seconds) {
  LostRecovery::Fields f;
  if (lost_.served(rec.relocalized, f)) reloc_request_.reset();
  rec.recovery_attempt = f.recovery_attempt;
  rec.recovery_succeeded = f.recovery_succeeded;
  if (f.recovery_attempt) {
    profile_["lost_recovery.attempts"] += 1.0;
    profile_["lost_recovery.seconds"] += seconds;
  }
  rec.bad_streak = lost_.badStreak();
}

void LidarOdometry::ensure_device() {
  if (raw_) return;
  if (!ctx_) ctx_ = DeviceContext::Default();
  raw_ = std::make_shared<DevicePointCloud>(ctx_);
  map_skewed_ = std::make_shared<DevicePointCloud>(ctx_);
  icp_skewed_ = std::make_shared<DevicePointCloud>(ctx_);
  for_map_ = std::make_shared<DevicePointCloud>(ctx_);
  for_icp_ = std::make_shared<DevicePointCloud>(ctx_);
}

uint64_t LidarOdometry::maps_total(bool voxels) const {  // general plans: all maps together
  uint64_t n = 0;
  for (const auto& m : gplan_->maps)
    if (m.map) n += voxels ? m.map->voxelCount() : m.map->size();
  return n;
}

void LidarOdometry::resolve_map_counts() const {
  if (!map_counts_pending_) return;
  if (gplan_) {
    map_points_cached_ = maps_total(false);
    map_voxels_cached_ = maps_total(true);
  } else {
    map_points_cached_ = local_map_ ? local_map_->size() : 0;  // (mh_map_get_info: waits for the update if it still runs)
    map_voxels_cached_ = local_map_ ? local_map_->voxelCount() : 0;
  }
  for (size_t i = map_counts_from_; i < records_.size(); i++) {
    if (records_[i].dropped || records_[i].waiting || records_[i].ignored) continue;  // (those returned before the map was looked at)
    records_[i].n_map_points = map_points_cached_;
    records_[i].n_map_voxels = map_voxels_cached_;
  }
  map_counts_pending_ = false;
  // what map_is_empty() answers from now on follows the device's own count (an update with far-voxel removal may leave
  // the map empty: local_map_->empty() is what the reference asks every scan, LidarOdometry.cpp:817)
  map_known_nonempty_ = map_points_cached_ != 0;
}

bool LidarOdometry::map_is_empty() {
  if (!local_map_) return true;
  if (map_known_nonempty_) return false;
  map_known_nonempty_ = gplan_ ? maps_total(false) != 0 : local_map_->size() != 0;  // (a metric map is empty when all its layers are)
  return !map_known_nonempty_;
}

void LidarOdometry::reset() {
  cancel_prefetch();
  map_counts_pending_ = false;
  map_counts_from_ = 0;
  map_points_cached_ = map_voxels_cached_ = 0;
  map_known_nonempty_ = false;
  navstate_.reset();
  live_cleaner_.reset();  // (online_map_cleaning: the ring goes with the maps)
  gyro_buf_.clear();      // (gyro_deskew: the samples, the drop count and the scan count start again)
  gyro_table_.reset();
  scans_gyro_deskewed_ = 0;
  local_map_.reset();
  if (gplan_) {
    for (auto& m : gplan_->maps) m.map.reset();
    for (auto& st : gplan_->steps) st.range[0] = st.range[1] = NAN;  // (remember_intensity_range starts again)
  }
  last_lidar_pose_ = CPose3D();
  last_icp_was_good_ = true;
  last_icp_quality_ = 0;
  last_obs_tim_.reset();
  sync_.clear();
  last_obs_tim_by_label_.clear();
  labelled_seen_ = merged_input_ = false;
  last_icp_timestamp_.reset();
  first_ever_timestamp_.reset();
  last_obs_timestamp_.reset();
  last_motion_model_output_.reset();
  adapt_thres_sigma_ = 0;
  estimated_sensor_max_range_.reset();
  instantaneous_sensor_max_range_.reset();
  distance_checker_local_map_.clear();
  localmap_check_removal_counter_ = 0;
  trajectory_.clear();
  records_.clear();
  initial_localization_done_ = false;
  reloc_request_.reset();
  lost_.reset();  // (TRACKING, the streaks and the counts zero)
  lost_pose_ = CPose3D();
  recovery_error_.clear();
  kf_store_.reset(loaded_keyframes_);  // (likewise: the store starts from the loaded file's frames again)
  place_index_.reset();                // (... and the place index follows it from its first frame)
  place_frames_seen_ = 0;
  loop_closer_.reset();  // (made again, and fed the loaded frames again, once the target maps are known)
  loop_pushed_ = 0;
  trajectory_anchor_.clear();
  kf_targets_known_ = false;  // (a loaded header is held against the plan's maps once they exist: check_loaded_keyframe_targets)
  if (!loaded_maps_.empty()) restore_loaded_maps();  // (the reference's reset() runs initialize() again: the file is loaded again)
}

void LidarOdometry::updatePipelineTwistVariables(const Twist& tw) {  // :1571-1579
  source_.updateVariable("vx", tw.vx); source_.updateVariable("vy", tw.vy); source_.updateVariable("vz", tw.vz);
  source_.updateVariable("wx", tw.wx); source_.updateVariable("wy", tw.wy); source_.updateVariable("wz", tw.wz);
}

void LidarOdometry::updatePipelineDynamicVariables() {  // :1581-1635
  updatePipelineTwistVariables(last_motion_model_output_ ? last_motion_model_output_->twist : Twist());
  const TPose3D p = last_lidar_pose_.asTPose();
  source_.updateVariable("robot_x", p.x); source_.updateVariable("robot_y", p.y); source_.updateVariable("robot_z", p.z);
  source_.updateVariable("robot_yaw", p.yaw); source_.updateVariable("robot_pitch", p.pitch); source_.updateVariable("robot_roll", p.roll);
  source_.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", adapt_thres_sigma_ != 0 ? adapt_thres_sigma_ : params_.initial_sigma);
  source_.updateVariable("ICP_ITERATION", 0);
  const auto& vars = source_.getVariableValues();
  for (const char* v : {"icp_iterations", "SENSOR_TIME_OFFSET", "twistCorrectionCount"})
    if (!vars.count(v)) source_.updateVariable(v, 0);
  if (estimated_sensor_max_range_) source_.updateVariable("ESTIMATED_SENSOR_MAX_RANGE", *estimated_sensor_max_range_);
  source_.updateVariable("INSTANTANEOUS_SENSOR_MAX_RANGE", instantaneous_sensor_max_range_ ? *instantaneous_sensor_max_range_ : 20.0);
  if (last_obs_timestamp_ && first_ever_timestamp_)
    source_.updateVariable("current_relative_timestamp", *last_obs_timestamp_ - *first_ever_timestamp_);
  source_.realize();
}

// bounding-box "radius" used by the sensor range estimate (:1503-1508, 1523-1527): float norms, like TPoint3Df::norm()
static double bbox_radius(const float mn[3], const float mx[3]) {
  const float a = std::sqrt((mx[0] * mx[0] + mx[1] * mx[1]) + mx[2] * mx[2]);
  const float b = std::sqrt((mn[0] * mn[0] + mn[1] * mn[1]) + mn[2] * mn[2]);
  return (double)std::max(a, b);
}

static mh_preprocess_params make_pp(double decim_map_res, double decim_icp_res, uint32_t min_points_to_filter, double range_min,
                                    double range_max, int32_t bbox_mode, const double bbox_min[3], const double bbox_max[3],
                                    int32_t timestamp_method, double time_offset, int32_t decim_map_method = MH_DECIMATE_FIRST_POINT,
                                    int32_t decim_icp_method = MH_DECIMATE_FIRST_POINT) {
  mh_preprocess_params pp;
  memset(&pp, 0, sizeof(pp));  // (compared bytewise with the parameters a prefetch used)
  pp.decim_map_resolution = (float)decim_map_res;
  pp.decim_icp_resolution = (float)decim_icp_res;
  pp.min_points_to_filter = min_points_to_filter;
  pp.index_mode = (int32_t)molahip_host::plugin_switches().index_mode;  // MOLA_HIP_INDEX_MODE (default floor)
  pp.range_min = (float)range_min;
  pp.range_max = (float)range_max;
  pp.bbox_mode = bbox_mode;
  for (int a = 0; a < 3; a++) {
    pp.bbox_min[a] = (float)bbox_min[a];
    pp.bbox_max[a] = (float)bbox_max[a];
  }
  pp.timestamp_method = timestamp_method;
  pp.time_offset = (float)time_offset;
  pp.decim_map_method = decim_map_method;
  pp.decim_icp_method = decim_icp_method;
  return pp;
}

// general plans: the buffer of 'raw' with adjusted time stamps lives in the layer table under a key no pipeline can name
// (downloadLayer() serves it as 'raw' and refuses the key itself)
static const char* const kAdjustedRawKey = " raw (time stamps adjusted)";

void LidarOdometry::run_general_pass(int pass) {
  GeneralPlan& g = *gplan_;
  const auto& v = source_.getVariableValues();
  auto layer = [&](const std::string& name) -> std::shared_ptr<DevicePointCloud> {
    if (name == "raw") return g.raw_adjusted ? g.raw_adjusted : cur_raw_;
    auto& b = g.buf[name];
    if (!b) b = std::make_shared<DevicePointCloud>(ctx_);
    return b;
  };
  if (pass == 1) {
    g.raw_adjusted.reset();
    // observations_filter_adjust_timestamps over all raw points (a rig's merged cloud: done per sensor by the merge)
    if (g.timestamp_method != MH_TS_NONE && !merged_input_) {
      const double zero[3] = {0, 0, 0};
      const mh_preprocess_params pp = make_pp(0, 0, 0, 0, 0, MH_BBOX_OFF, zero, zero, g.timestamp_method, g.time_offset);
      auto out = layer(kAdjustedRawKey);
      check(mh_scan_preprocess(cur_raw_->handle(), &pp, out->handle(), nullptr), "mh_scan_preprocess (adjust time stamps)");
      g.raw_adjusted = out;
    }
    g.alive = {"raw"};
    if (g.depth_input) g.alive = {g.steps[0].out[0], g.steps[0].out[1]};  // what the generator wrote at upload
  } else {
    g.alive = g.alive_1st;  // (the twist hook runs this pass again from the same start)
  }
  for (auto& st : g.steps) {
    if (st.pass != pass) continue;
    using K = GeneralPlan::Kind;
    if (st.kind == K::Delete) {
      for (const auto& n : st.out) g.alive.erase(n);
      continue;
    }
    if (!g.alive.count(st.in)) throw std::runtime_error("LidarOdometry (HIP): " + st.cls + " reads the deleted layer '" + st.in + "'");
    mh_scan* in = layer(st.in)->handle();
    if (st.kind == K::NormalizeIntensity) {  // (in place: the remembered range lives in the step, per step)
      check(mh_scan_normalize_intensity(in, st.remember_range ? st.range : nullptr), "mh_scan_normalize_intensity");
    } else if (st.kind == K::ByIntensity) {
      mh_by_intensity_params bp;
      memset(&bp, 0, sizeof(bp));
      bp.low_threshold = (float)st.low_threshold;
      bp.high_threshold = (float)st.high_threshold;
      mh_scan* o[3];
      for (int k = 0; k < 3; k++) o[k] = st.out[k].empty() ? nullptr : layer(st.out[k])->handle();
      check(mh_scan_by_intensity(in, &bp, o[0], o[1], o[2]), "mh_scan_by_intensity");
    } else if (st.kind == K::Deskew) {
      const double tw[6] = {v.at("vx"), v.at("vy"), v.at("vz"), v.at("wx"), v.at("wy"), v.at("wz")};
      if (gyro_table_ && !st.skip_deskew) {  // gyro_deskew: the measured rotations of this sweep, the current v
        for (int a = 0; a < 3; a++) gyro_table_->v[a] = tw[a];
        const mh_motion_table mt = gyro_table_->table();
        check(mh_scan_deskew_motion(in, &mt, layer(st.out[0])->handle()), "mh_scan_deskew_motion");
      } else {
        check(mh_scan_deskew(in, st.skip_deskew ? nullptr : tw, layer(st.out[0])->handle()), "mh_scan_deskew");
      }
    } else if (st.kind == K::Preprocess) {
      const mh_preprocess_params pp = make_pp(st.res, 0, st.min_points, st.range_min, st.range_on ? st.range_max : 0, st.bbox_mode,
                                              st.bbox_min, st.bbox_max, MH_TS_NONE, 0, st.method);
      check(mh_scan_preprocess(in, &pp, layer(st.out[0])->handle(), nullptr), "mh_scan_preprocess");
    } else {
      mh_curvature_params cp;
      memset(&cp, 0, sizeof(cp));
      cp.max_cosine = (float)st.max_cosine;
      cp.min_clearance = (float)st.min_clearance;
      cp.max_gap = (float)st.max_gap;
      mh_scan* o[3];
      for (int k = 0; k < 3; k++) o[k] = st.out[k].empty() ? nullptr : layer(st.out[k])->handle();
      check(mh_scan_curvature(in, &cp, o[0], o[1], o[2]), "mh_scan_curvature");
    }
    for (const auto& n : st.out)
      if (!n.empty()) g.alive.insert(n);
  }
  if (pass == 1) {
    g.alive_1st = g.alive;
  } else {
    // the sensor-range estimate reads the alphabetically first point layer of the observation (LidarOdometry.cpp:1515-1545)
    // (depth images: the union box of the generator's layers -- all point layers of the observation as it arrived)
    for (int a = 0; a < 3; a++) icp_bb_min_[a] = g.depth_input ? g.gen_bb_min[a] : 0.f, icp_bb_max_[a] = g.depth_input ? g.gen_bb_max[a] : 0.f;
    if (!g.depth_input && !g.alive.empty()) layer(*g.alive.begin())->boundingBox(icp_bb_min_, icp_bb_max_);
  }
}

void LidarOdometry::record_layer_sizes(ScanRecord& rec) const {
  rec.layer_sizes.clear();
  rec.n_for_icp = rec.n_for_map = 0;
  for (const auto& name : gplan_->alive) {
    const uint64_t k = (name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name))->size();
    rec.layer_sizes[name] = k;
    rec.n_for_icp += k;
  }
  for (const auto& [name, m] : gplan_->merges)
    if (rec.layer_sizes.count(name)) rec.n_for_map += rec.layer_sizes[name];
}

void LidarOdometry::run_first_pass() {
  if (gplan_) return run_general_pass(1);
  const FilterPlan& f = *plan_;
  const mh_preprocess_params pp = make_pp(f.decim_map_res, f.decim_icp_res, f.min_points_to_filter, f.range_min, f.range_max,
                                          f.bbox_mode, f.bbox_min, f.bbox_max, merged_input_ ? (int32_t)MH_TS_NONE : f.timestamp_method,
                                          f.time_offset, f.decim_map_method, f.decim_icp_method);  // (a rig's merged cloud: adjusted per sensor)
  // (not through the batcher even when there is one: its filter sets are made of the PREFETCH requests, one action per
  // alignment and participant -- this call is the first scan of a sequence, or a prepared scan that has to be redone)
  check(mh_scan_preprocess(raw_->handle(), &pp, map_skewed_->handle(), icp_skewed_->handle()), "mh_scan_preprocess");
}

void LidarOdometry::setAlignBatcher(std::shared_ptr<mp2p_icp_hip::AlignBatcher> b) {
  // the instances of a batch run on their own host threads: each needs a context (stream + scratch) of its own, the
  // process-wide default one would be shared between threads (molahip.h: one context, one thread at a time)
  // (general plans too: their ICP joins through whichever route it takes -- mp2p_icp_hip::ICP::align; their filter steps and
  // their next scan's upload are not announced to the batcher, launch_prefetch() is the default plan's)
  if (b && loop_enabled_)
    throw std::runtime_error("LidarOdometry::setAlignBatcher: not available with online_loop_closure: enabled (the batch protocol of an "
                             "AlignBatcher has no slot for the extra alignments that verify a loop)");
  if (b && lost_.options().enabled)
    throw std::runtime_error(std::string("LidarOdometry::setAlignBatcher: not available with lost_recovery: ") + kNoRecoveryWithBatcher);
  if (b && live_opts_.enabled)
    throw std::runtime_error(std::string("LidarOdometry::setAlignBatcher: not available with online_map_cleaning: ") + kNoLiveCleaningWithBatcher);
  if (b && gyro_opts_.enabled)
    throw std::runtime_error(std::string("LidarOdometry::setAlignBatcher: not available with gyro_deskew: ") + kNoGyroDeskewWithBatcher);
  if (b && (!ctx_ || ctx_ == DeviceContext::Default()))
    throw std::runtime_error("LidarOdometry::setAlignBatcher: this instance uses the process-wide default context; construct "
                             "it with a DeviceContext of its own");
  for (auto& i : icp_)
    if (i) i->setAlignBatcher(b, this);  // (both ICP objects align for this one participant)
  batcher_ = std::move(b);
}

// ---- the announced next observation: upload + first pass on a second stream while this scan is in its ICP loop
void LidarOdometry::refuse_unlabelled(const char* what) const {
  if (params_.lidar_count > 1)
    throw std::runtime_error(std::string("LidarOdometry (HIP): ") + what + " on a rig (params.multiple_lidars.lidar_count = " +
                             std::to_string(params_.lidar_count) + "): its observations carry a sensor label, use onLidarFrom");
}

void LidarOdometry::prefetch(const float* x, const float* y, const float* z, const float* t, size_t n) {
  refuse_unlabelled("prefetch");
  if (labelled_seen_) throw std::runtime_error("LidarOdometry (HIP): prefetch after a labelled observation (onLidarFrom): prefetch overlap for rigs is not implemented");
  pf_->req = RawInput();  // (a prepared scan that is still waiting to be picked up stays untouched)
  pf_->req.n = n; pf_->req.x = x; pf_->req.y = y; pf_->req.z = z; pf_->req.t = t;
  pf_->requested = n > 0;
}

void LidarOdometry::prefetchInterleaved(const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                                        size_t off_z, long long off_t, const float* t, long long off_i) {
  refuse_unlabelled("prefetchInterleaved");
  if (labelled_seen_) throw std::runtime_error("LidarOdometry (HIP): prefetchInterleaved after a labelled observation (onLidarFrom): prefetch overlap for rigs is not implemented");
  pf_->req = RawInput();
  pf_->req.n = n; pf_->req.data = data; pf_->req.point_step = point_step; pf_->req.off_x = off_x; pf_->req.off_y = off_y;
  pf_->req.off_z = off_z; pf_->req.off_t = off_t; pf_->req.t = t; pf_->req.off_i = off_i;
  pf_->requested = n > 0;
}

void LidarOdometry::cancel_prefetch() {
  if (pf_->launched) {
    try { pf_->join(); } catch (...) {}
  }
  pf_->launched = pf_->requested = false;
}

void LidarOdometry::launch_prefetch() {
  if (!pf_->requested || !plan_ || !estimated_sensor_max_range_) {
    return;  // (the last scan of the sequence, or nothing announced: the batcher sees this sequence's next alignment)
  }
  if (pf_->launched) {  // prepared but never picked up: drop it
    try { pf_->join(); } catch (...) {}
    pf_->launched = false;
  }
  pf_->in = pf_->req;
  if (!ctx_b_) {
    // the next scan's upload and filters run beside the current alignment on a stream of their own.  (Measured in round 3 and
    // removed in round 4: a stream of the LOW priority class -- 8 sequences 2180 scans/s against 2870 -- and a stream
    // restricted to a quarter or an eighth of the compute units -- 4530-4650 against 4780: whatever the filters and uploads
    // take from the alignment's kernels, it is neither dispatch priority nor wave slots.)
    ctx_b_ = std::make_shared<DeviceContext>(ctx_->device());
    for (int i = 0; i < 2; i++) {
      raw_b_[i] = std::make_shared<DevicePointCloud>(ctx_b_);
      map_skewed_b_[i] = std::make_shared<DevicePointCloud>(ctx_b_);
      icp_skewed_b_[i] = std::make_shared<DevicePointCloud>(ctx_b_);
    }
  }
  pf_->slot ^= 1;  // not the set the current scan may still be reading
  // the filter parameters as the next onLidar will publish them (:692): only the sensor range differs from now
  std::map<std::string, double> vars = source_.getVariableValues();
  vars["ESTIMATED_SENSOR_MAX_RANGE"] = *estimated_sensor_max_range_;
  vars["INSTANTANEOUS_SENSOR_MAX_RANGE"] = instantaneous_sensor_max_range_ ? *instantaneous_sensor_max_range_ : 20.0;
  plan_->realizeWith(vars);
  const FilterPlan& f = *plan_;
  pf_->pp = make_pp(f.decim_map_res, f.decim_icp_res, f.min_points_to_filter, f.range_min, f.range_max, f.bbox_mode,
                    f.bbox_min, f.bbox_max, f.timestamp_method, f.time_offset, f.decim_map_method, f.decim_icp_method);
  plan_->realizeWith(source_.getVariableValues());  // and back: this scan goes on with what it started with
  const RawInput in = pf_->in;
  const mh_preprocess_params pp = pf_->pp;
  auto raw = raw_b_[pf_->slot], ms = map_skewed_b_[pf_->slot], is = icp_skewed_b_[pf_->slot];
  auto ctx = ctx_b_;
  const bool pinned = input_pinned_;
  auto batcher = batcher_;
  const void* owner = this;
  // several sequences in one process: the request is announced HERE, on the thread that aligns next (the batcher then
  // knows it is coming before it sees that alignment), and delivered by the worker
  const size_t filter_set = batcher ? batcher->announceFilter(owner) : 0;
  auto work = [in, pp, raw, ms, is, ctx, pinned, batcher, owner, filter_set]() {
    bool delivered = false;
    try {
      if (in.data) raw->setPointsInterleaved(in.data, in.n, in.point_step, in.off_x, in.off_y, in.off_z, in.off_t, pinned);
      else raw->setPoints(in.x, in.y, in.z, in.n);
      if (in.t) raw->setTimestamps(in.t, in.n);
      if (batcher) {
        std::string err;
        delivered = true;
        const mh_status st = batcher->preprocess(owner, filter_set, raw->handle(), &pp, ms->handle(), is->handle(), &err);
        if (st != MH_OK) throw std::runtime_error("mh_scan_preprocess (prefetch, batched): " + err);
      } else {
        check(mh_scan_preprocess(raw->handle(), &pp, ms->handle(), is->handle()), "mh_scan_preprocess (prefetch)");
      }
      ctx->synchronize();
    } catch (...) {
      if (batcher && !delivered) batcher->cancelAnnouncedFilter(owner, filter_set);  // (the others must not wait for it)
      throw;
    }
  };
  pf_->worker.submit(work);
  pf_->on_worker = true;
  pf_->launched = true;
  pf_->requested = false;
}

void LidarOdometry::run_second_pass() {
  if (gplan_) return run_general_pass(2);
  const auto& v = source_.getVariableValues();
  const double tw[6] = {v.at("vx"), v.at("vy"), v.at("vz"), v.at("wx"), v.at("wy"), v.at("wz")};
  const double* twp = plan_->skip_deskew ? nullptr : tw;
  if (gyro_table_ && twp) {  // gyro_deskew: the measured rotations of this sweep, the current v
    for (int a = 0; a < 3; a++) gyro_table_->v[a] = tw[a];
    const mh_motion_table mt = gyro_table_->table();
    check(mh_scan_deskew_motion_pair(cur_map_skewed_->handle(), cur_icp_skewed_->handle(), &mt, for_map_->handle(), for_icp_->handle(),
                                     icp_bb_min_, icp_bb_max_, nullptr), "mh_scan_deskew_motion_pair");
    return;
  }
  // both layers and the bounding box of the de-skewed ICP layer (read by the sensor-range estimate right below) at once
  check(mh_scan_deskew_pair(cur_map_skewed_->handle(), cur_icp_skewed_->handle(), twp, for_map_->handle(), for_icp_->handle(),
                            icp_bb_min_, icp_bb_max_, nullptr), "mh_scan_deskew_pair");
}

void LidarOdometry::doUpdateAdaptiveThreshold(const CPose3D& err) {  // :1449-1485 (KISS-ICP's scheme)
  if (!estimated_sensor_max_range_) return;
  const double max_range = *estimated_sensor_max_range_;
  const double theta = err.rotationAngle();
  const double model_error = err.translationNorm() + 2.0 * max_range * std::sin(theta / 2.0);
  double rot_error = 0;
  if (last_motion_model_output_) {
    const Twist& tw = last_motion_model_output_->twist;
    rot_error = 0.1 * std::sqrt(tw.wx * tw.wx + tw.wy * tw.wy + tw.wz * tw.wz) * max_range;
  }
  const double KP = params_.kp;
  if (!(KP > 1.0)) throw std::runtime_error("adaptive_threshold.kp must be > 1");
  const double gain = std::min(KP, std::max(0.1, KP * (1.0 - last_icp_quality_)));
  const double new_sigma = (model_error + rot_error) * gain;
  if (adapt_thres_sigma_ == 0) adapt_thres_sigma_ = params_.initial_sigma;
  adapt_thres_sigma_ = params_.alpha * adapt_thres_sigma_ + (1.0 - params_.alpha) * new_sigma;
  adapt_thres_sigma_ = std::min(params_.maximum_sigma, std::max(params_.min_motion, adapt_thres_sigma_));
}

void LidarOdometry::create_local_map() {  // :1165-1171 with yaml:228-242
  if (gplan_) {  // one map per localmap_generator entry; local_map_ = the first (localMap(), the ICP schedule)
    for (auto& m : gplan_->maps) m.map = make_map(m.def, &m.voxel_size, &m.remove_far);
    local_map_ = gplan_->maps[0].map;
    map_voxel_size_ = gplan_->maps[0].voxel_size;
    return;
  }
  local_map_ = make_map(map_def_, &map_voxel_size_, &remove_voxels_farther_than_);
}

std::shared_ptr<HashedVoxelPointCloud> LidarOdometry::make_map(const Config& def, double* voxel_size, float* remove_far) const {
  const auto& vars = source_.getVariableValues();
  const std::string cls = def["class"].asString();
  const Config& co = def["creationOpts"];
  const Config& io = def["insertOpts"];
  if (ends_with(cls, "CVoxelMap")) {  // mrpt::maps::CVoxelMap (lidar2d.yaml:183-198): the occupancy voxel map
    auto num = [&](const Config& c, const char* key, double dflt) { return c.has(key) ? eval_now(c[key].asString(), vars) : dflt; };
    mh_occmap_params op = mp2p_icp_hip::CVoxelMap::defaultParams(0.f);
    *voxel_size = num(co, "resolution", 0.20);
    op.resolution = (float)*voxel_size;
    op.prob_hit = (float)num(io, "prob_hit", op.prob_hit);
    op.prob_miss = (float)num(io, "prob_miss", op.prob_miss);
    op.clamp_min = (float)num(io, "clamp_min", op.clamp_min);
    op.clamp_max = (float)num(io, "clamp_max", op.clamp_max);
    if (io.has("ray_trace_free_space")) op.ray_trace_free_space = to_bool(io["ray_trace_free_space"].asString()) ? 1u : 0u;
    op.decimation = (uint32_t)std::max(1.0, num(io, "decimation", 1.0));
    op.max_range = (float)std::max(0.0, num(io, "max_range", 0.0));
    if (def.has("likelihoodOpts")) op.occupied_threshold = (float)num(def["likelihoodOpts"], "occupiedThreshold", op.occupied_threshold);
    *remove_far = (float)num(io, "remove_voxels_farther_than", 0.0);
    return std::make_shared<mp2p_icp_hip::CVoxelMap>(op, ctx_);
  }
  if (ends_with(cls, "SparseTreesPointCloud")) {  // mola::SparseTreesPointCloud (rgbd.yaml:203-217): an uncapped map whose voxel is the cell
    auto num = [&](const Config& c, const char* key, double dflt) { return c.has(key) ? eval_now(c[key].asString(), vars) : dflt; };
    *voxel_size = num(co, "grid_size", 10.0);
    *remove_far = (float)num(io, "remove_submaps_farther_than", 0.0);
    return std::make_shared<mp2p_icp_hip::SparseTreesPointCloud>((float)*voxel_size, (float)num(io, "minimum_points_clearance", 0.0), ctx_);
  }
  mh_map_params mp{};
  *voxel_size = eval_now(co["voxel_size"].asString(), vars);
  mp.voxel_size = (float)*voxel_size;
  mp.max_points_per_voxel = io.has("max_points_per_voxel") ? (uint32_t)eval_now(io["max_points_per_voxel"].asString(), vars) : 0;
  mp.index_mode = molahip_host::plugin_switches().index_mode;
  mp.far_voxel_metric = molahip_host::plugin_switches().far_voxel_metric;  // MOLA_HIP_FAR_VOXEL_METRIC
  mp.min_distance_between_points = io.has("min_distance_between_points") ? (float)eval_now(io["min_distance_between_points"].asString(), vars) : 0.f;
  *remove_far = io.has("remove_voxels_farther_than") ? (float)eval_now(io["remove_voxels_farther_than"].asString(), vars) : 0.f;
  if (ends_with(cls, "NDT")) {
    mp.ndt_max_eigen_ratio = io.has("max_eigen_ratio_for_planes") ? (float)eval_now(io["max_eigen_ratio_for_planes"].asString(), vars) : 0.05f;
    mp.ndt_min_points = 4;
  } else if (!ends_with(cls, "HashedVoxelPointCloud")) {
    throw std::runtime_error("local map class '" + cls + "' has no device implementation (HashedVoxelPointCloud, NDT, CVoxelMap, SparseTreesPointCloud)");
  }
  return std::make_shared<HashedVoxelPointCloud>(mp, ctx_);
}

const LidarOdometry::ScanRecord& LidarOdometry::onLidar(double this_obs_tim, const float* x, const float* y, const float* z,
                                                        const float* t, size_t n) {
  refuse_unlabelled("onLidar");
  RawInput in;
  in.n = n; in.x = x; in.y = y; in.z = z; in.t = t;
  return process(this_obs_tim, in);
}

const LidarOdometry::ScanRecord& LidarOdometry::onLidarInterleaved(double this_obs_tim, const void* data, size_t n,
                                                                   size_t point_step, size_t off_x, size_t off_y,
                                                                   size_t off_z, long long off_t, const float* t, long long off_i) {
  refuse_unlabelled("onLidarInterleaved");
  RawInput in;
  in.n = n; in.data = data; in.point_step = point_step; in.off_x = off_x; in.off_y = off_y; in.off_z = off_z;
  in.off_t = off_t; in.t = t; in.off_i = off_i;
  return process(this_obs_tim, in);
}

void LidarOdometry::merge_sensors(const std::vector<std::string>& labels, const std::vector<mh_merge_source>& srcs, DevicePointCloud& out) {
  const mh_scan* scans[MH_MAX_MERGE_SOURCES];
  for (size_t k = 0; k < labels.size(); k++) scans[k] = sensors_.at(labels[k]).cloud->handle();
  check(mh_scan_merge_sensors(labels.size(), scans, srcs.data(), out.handle()), "mh_scan_merge_sensors");
}

const LidarOdometry::ScanRecord& LidarOdometry::onLidarFrom(const std::string& label, const double* sensor_pose, double this_obs_tim,
                                                            const void* data, size_t n, size_t point_step, size_t off_x,
                                                            size_t off_y, size_t off_z, long long off_t, const float* t,
                                                            long long off_i) {
  if (!plan_ && !gplan_) throw std::runtime_error("LidarOdometry::onLidarFrom called before initialize()");
  if (gplan_ && gplan_->depth_input)
    throw std::runtime_error("LidarOdometry (HIP): this pipeline's observations_generator is a GeneratorEdgesFromRangeImage: it "
                             "takes depth images (onDepthImage), not point clouds");
  const bool with_i = gplan_ && gplan_->reads_intensity;
  if (with_i && off_i < 0)
    throw std::runtime_error("LidarOdometry (HIP): the pipeline's intensity filters need a per-point intensity, and this scan "
                             "carries none (onLidarFrom with off_i >= 0)");
  auto side_record = [&]() -> ScanRecord& {  // a record of an observation that does not become a scan
    records_.emplace_back();
    ScanRecord& r = records_.back();
    r.timestamp = this_obs_tim;
    r.n_raw = n;
    r.pose = last_lidar_pose_;
    r.n_sensors = 0;
    r.sensor_labels = {label};
    return r;
  };
  // 1. is it a LiDAR of ours? (:576-577)
  if (!label_patterns_.empty()) {
    bool ours = false;
    for (const auto& re : label_patterns_) ours = ours || std::regex_match(label, re);
    if (!ours) {
      ScanRecord& r = side_record();
      r.ignored = true;
      return r;
    }
  }
  // 2. observations of one label too close in time (:644-657).  NOTE the reference records the time under the label of the
  // observation that COMPLETES a group only, and only after the validity check (:763): a sensor whose observations always
  // wait is never dropped by this test.  Kept (process() writes last_obs_tim_by_label_ for the triggering label).
  if (auto it = last_obs_tim_by_label_.find(label); it != last_obs_tim_by_label_.end() && (this_obs_tim - it->second) < params_.min_time_between_scans) {
    ScanRecord& r = side_record();
    r.dropped = true;
    return r;
  }
  if (!labelled_seen_) cancel_prefetch();  // (an announced unlabelled scan: from here on the driver is fed by label)
  labelled_seen_ = true;
  ensure_device();
  // 3. the observation goes to the device at once, in its sensor frame, stamps untouched; a newer one replaces a waiting one
  SensorSlot& slot = sensors_[label];
  {
    StageTimer tt(profile_, "onLidar.0.upload_raw");
    if (!slot.cloud) slot.cloud = std::make_shared<DevicePointCloud>(ctx_);
    slot.cloud->setPointsInterleaved(data, n, point_step, off_x, off_y, off_z, off_t, input_pinned_, with_i ? off_i : -1);
    if (t) slot.cloud->setTimestamps(t, n);
    for (int c = 0; c < 12; c++) slot.pose[c] = sensor_pose ? sensor_pose[c] : (c % 5 == 0 ? 1.0 : 0.0);
  }
  auto source_of = [&](const std::string& l, int32_t method, double offset) {
    mh_merge_source m;
    memset(&m, 0, sizeof(m));
    for (int c = 0; c < 12; c++) m.sensor_pose[c] = sensors_.at(l).pose[c];
    m.timestamp_method = method;
    m.time_offset = (float)offset;
    return m;
  };
  // 4. first call: the sensor range from this one observation in the vehicle frame (:662, 1487-1513), even if it then waits
  if (!estimated_sensor_max_range_ && n) {
    if (!range_probe_) range_probe_ = std::make_shared<DevicePointCloud>(ctx_);
    merge_sensors({label}, {source_of(label, MH_TS_NONE, 0)}, *range_probe_);
    float mn[3], mx[3];
    range_probe_->boundingBox(mn, mx);
    estimated_sensor_max_range_ = std::max(bbox_radius(mn, mx), params_.absolute_minimum_sensor_range);
    updatePipelineDynamicVariables();  // (the estimate is published now, as the next observation's :692 would)
  }
  // 5. / 6. the group (:664-689)
  const std::optional<SensorSync::Group> group = sync_.push(label, this_obs_tim);
  if (!group) {
    ScanRecord& r = side_record();
    r.waiting = true;
    return r;
  }
  // 7. one merge into 'raw': sensor poses, and FilterAdjustTimestamps per source with ITS SENSOR_TIME_OFFSET (:692, 704-721)
  updatePipelineDynamicVariables();
  const int32_t method = plan_ ? plan_->timestamp_method : gplan_->timestamp_method;
  std::vector<mh_merge_source> srcs;
  for (size_t k = 0; k < group->labels.size(); k++) {
    source_.updateVariable("SENSOR_TIME_OFFSET", group->dts[k]);  // (keeps the last source's value afterwards, :713)
    source_.realize();
    srcs.push_back(source_of(group->labels[k], method, plan_ ? plan_->time_offset : gplan_->time_offset));
  }
  {
    StageTimer tt(profile_, "onLidar.0.merge_sensors");
    merge_sensors(group->labels, srcs, *raw_);
  }
  RawInput in;
  in.n = raw_->size();
  in.merged_labels = &group->labels;
  in.trigger_label = &label;
  return process(this_obs_tim, in);
}

const LidarOdometry::ScanRecord& LidarOdometry::onDepthImage(double this_obs_tim, const uint16_t* range,
                                                             const mh_range_image_params& camera) {
  if (!range || !camera.rows || !camera.cols) throw std::runtime_error("LidarOdometry::onDepthImage: empty image");
  RawInput in;
  in.depth = range;
  in.cam = camera;
  in.n = (size_t)camera.rows * camera.cols;
  return process(this_obs_tim, in);
}

// observations_generator of a depth-image plan: the image goes up (asynchronously from page-locked memory, setInputPinned)
// and leaves the generator's two layers; their union bounding box feeds the sensor-range estimate
void LidarOdometry::run_generator(const RawInput& in) {
  GeneralPlan& g = *gplan_;
  const GeneralPlan::Step& st = g.steps[0];
  mh_range_image_params cam = in.cam;
  cam.row_window_length = st.row_window_length;  // (the pipeline's values, whatever the caller left there)
  cam.score_threshold = (float)st.score_threshold;
  std::shared_ptr<DevicePointCloud> out[2];
  for (int k = 0; k < 2; k++) {
    auto& b = g.buf[st.out[k]];
    if (!b) b = std::make_shared<DevicePointCloud>(ctx_);
    out[k] = b;
  }
  check(mh_scan_edges_from_range_image(ctx_->get(), in.depth, input_pinned_ ? MH_MEM_HOST_PINNED : MH_MEM_HOST, &cam,
                                       out[0]->handle(), out[1]->handle()), "mh_scan_edges_from_range_image");
  bool any = false;
  for (int k = 0; k < 2; k++) {
    if (!out[k]->size()) continue;
    float mn[3], mx[3];
    out[k]->boundingBox(mn, mx);
    for (int a = 0; a < 3; a++) {
      g.gen_bb_min[a] = any ? std::min(g.gen_bb_min[a], mn[a]) : mn[a];
      g.gen_bb_max[a] = any ? std::max(g.gen_bb_max[a], mx[a]) : mx[a];
    }
    any = true;
  }
  if (!any)
    for (int a = 0; a < 3; a++) g.gen_bb_min[a] = g.gen_bb_max[a] = 0.f;
}

const LidarOdometry::ScanRecord& LidarOdometry::process(double this_obs_tim, const RawInput& in) {
  const size_t n = in.n;
  const bool has_t = in.t != nullptr || (in.data && in.off_t >= 0);
  (void)has_t;
  if (!plan_ && !gplan_) throw std::runtime_error("LidarOdometry::onLidar called before initialize()");
  if (in.depth && !(gplan_ && gplan_->depth_input))
    throw std::runtime_error("LidarOdometry (HIP): onDepthImage needs a pipeline whose observations_generator is a "
                             "GeneratorEdgesFromRangeImage; this one takes point clouds (onLidar / onLidarInterleaved)");
  if (!in.depth && gplan_ && gplan_->depth_input)
    throw std::runtime_error("LidarOdometry (HIP): this pipeline's observations_generator is a GeneratorEdgesFromRangeImage: it "
                             "takes depth images (onDepthImage), not point clouds");
  const bool merged = in.merged_labels != nullptr;  // a rig's group: 'raw' is on the device already, adjusted per sensor
  merged_input_ = merged;
  // 'raw' carries the intensity only when a filter reads it: otherwise the field is ignored (same records as without it)
  const bool with_i = gplan_ && gplan_->reads_intensity;
  if (with_i && !merged && !(in.data && in.off_i >= 0))
    throw std::runtime_error("LidarOdometry (HIP): the pipeline's intensity filters need a per-point intensity, and this scan "
                             "carries none (onLidarInterleaved with off_i >= 0)");
  const long long off_i = with_i ? in.off_i : -1;
  records_.emplace_back();
  ScanRecord& rec = records_.back();
  rec.timestamp = this_obs_tim;
  rec.n_raw = n;
  rec.pose = last_lidar_pose_;
  if (merged) {
    rec.n_sensors = (uint32_t)in.merged_labels->size();
    rec.sensor_labels = *in.merged_labels;
  }

  // drop scans too close in time (:644-657; labelled observations: per label, in onLidarFrom)
  if (!merged && last_obs_tim_ && (this_obs_tim - *last_obs_tim_) < params_.min_time_between_scans) {
    rec.dropped = true;
    return rec;
  }
  StageTimer t_all(profile_, "onLidar");
  ensure_device();
  cur_raw_ = raw_;
  cur_map_skewed_ = map_skewed_;
  cur_icp_skewed_ = icp_skewed_;
  bool prepared = false;  // upload + first pass already done by the prefetch worker?
  if (pf_->launched) {
    StageTimer tt(profile_, "onLidar.0.prefetch_wait");
    bool ok = true;
    try { pf_->join(); } catch (...) { ok = false; }  // (a failed prefetch is simply redone below, and reports there)
    pf_->launched = false;
    if (ok && pf_->in.same(in)) prepared = true;
  }
  if (pf_->requested && pf_->req.same(in)) pf_->requested = false;  // due before it could be launched
  if (!prepared && !merged) {
    StageTimer tt(profile_, "onLidar.0.upload_raw");
    if (in.depth) run_generator(in);
    else if (in.data) raw_->setPointsInterleaved(in.data, n, in.point_step, in.off_x, in.off_y, in.off_z, in.off_t, input_pinned_, off_i);
    else raw_->setPoints(in.x, in.y, in.z, n);
    if (in.t) raw_->setTimestamps(in.t, n);
  }

  // first call: sensor range from the raw cloud (:660, 1487-1513)
  if (!estimated_sensor_max_range_ && n) {
    float mn[3], mx[3];
    if (in.depth) {
      for (int a = 0; a < 3; a++) mn[a] = gplan_->gen_bb_min[a], mx[a] = gplan_->gen_bb_max[a];
    } else {
      cur_raw_->boundingBox(mn, mx);
    }
    estimated_sensor_max_range_ = std::max(bbox_radius(mn, mx), params_.absolute_minimum_sensor_range);
  }
  {
    StageTimer tt(profile_, "onLidar.0.dynamic_variables");
    updatePipelineDynamicVariables();  // :692
  }
  rec.twist = last_motion_model_output_ ? last_motion_model_output_->twist : Twist();

  if (prepared) {  // valid only if the parameters published just now are the ones the worker used
    const FilterPlan& f = *plan_;
    const mh_preprocess_params now = make_pp(f.decim_map_res, f.decim_icp_res, f.min_points_to_filter, f.range_min, f.range_max,
                                             f.bbox_mode, f.bbox_min, f.bbox_max, f.timestamp_method, f.time_offset, f.decim_map_method, f.decim_icp_method);
    if (memcmp(&now, &pf_->pp, sizeof(now)) == 0) {
      cur_raw_ = raw_b_[pf_->slot];
      cur_map_skewed_ = map_skewed_b_[pf_->slot];
      cur_icp_skewed_ = icp_skewed_b_[pf_->slot];
      profile_["prefetch_hits"] += 1.0;
    } else {
      prepared = false;
      profile_["prefetch_misses"] += 1.0;
      StageTimer tt(profile_, "onLidar.0.upload_raw");
      if (in.data) raw_->setPointsInterleaved(in.data, n, in.point_step, in.off_x, in.off_y, in.off_z, in.off_t, input_pinned_, off_i);
      else raw_->setPoints(in.x, in.y, in.z, n);
      if (in.t) raw_->setTimestamps(in.t, n);
    }
  }
  gyro_table_.reset();
  // gyro_deskew: the rotations of this sweep, once per scan and before either pass (a general plan may de-skew in its first; the
  // twist hook changes v only)
  if (gyro_opts_.enabled && (merged || has_t)) {
    bool deskews = plan_ && !plan_->skip_deskew;  // (skip_deskew wins over the block; a scan without stamps is copied either way)
    if (gplan_)
      for (const auto& st : gplan_->steps) deskews = deskews || (st.kind == GeneralPlan::Kind::Deskew && !st.skip_deskew);
    const double zero[3] = {0, 0, 0};
    if (deskews) gyro_table_ = build_motion_table(gyro_buf_, this_obs_tim, gyro_opts_, zero);
  }
  if (!prepared) {
    StageTimer tt(profile_, "onLidar.1.filter_1st");
    run_first_pass();  // :734
  }
  {
    StageTimer tt(profile_, "onLidar.1.filter_2nd");
    run_second_pass();  // :739
  }
  if (gyro_table_) {
    rec.gyro_deskew = true;
    rec.gyro_segments = (uint32_t)gyro_table_->segments.size();
    scans_gyro_deskewed_++;
  }
  if (gplan_) {
    record_layer_sizes(rec);
  } else {
    rec.decim_map_resolution = plan_->decim_map_res;
    rec.decim_icp_resolution = plan_->decim_icp_res;
    rec.n_for_map = for_map_->size();
    rec.n_for_icp = for_icp_->size();
  }

  // sensor range low-pass from the first point layer of the observation, 'decimated_for_icp' (:744, 1515-1545)
  if (estimated_sensor_max_range_) {
    StageTimer tt(profile_, "onLidar.2.sensor_range");
    const double radius = std::max(bbox_radius(icp_bb_min_, icp_bb_max_), params_.absolute_minimum_sensor_range);  // (run_second_pass)
    instantaneous_sensor_max_range_ = radius;
    const double a = params_.max_sensor_range_filter_coefficient;
    estimated_sensor_max_range_ = *estimated_sensor_max_range_ * a + radius * (1.0 - a);
  }
  launch_prefetch();  // the announced next scan: its first pass only needs the range estimate, which is final now
  rec.estimated_sensor_max_range = estimated_sensor_max_range_.value_or(0);
  rec.instantaneous_sensor_max_range = instantaneous_sensor_max_range_.value_or(0);

  if (params_.validity_check_enabled && !(n > params_.validity_minimum_point_count)) {  // :749-757, 1548-1568
    rec.dropped = true;
    return rec;
  }
  if (merged) last_obs_tim_by_label_[*in.trigger_label] = this_obs_tim;  // (:763: the label that completed the group only)
  else last_obs_tim_ = this_obs_tim;
  last_obs_timestamp_ = this_obs_tim;
  if (!first_ever_timestamp_) first_ever_timestamp_ = this_obs_tim;
  if (n == 0) {  // :769-775
    rec.dropped = true;
    return rec;
  }

  // initial localization (:779-794), once, at the first observation that reaches registration
  if (init_loc_.enabled && !initial_localization_done_) {
    const CPose3D fixed(init_loc_.fixed_initial_pose);
    if (init_loc_.relocalize) {  // this implementation's extension: search around the fixed pose
      double cov[36] = {0};
      cov[0] = init_loc_.relocalize_sigmas[0] * init_loc_.relocalize_sigmas[0];
      cov[7] = init_loc_.relocalize_sigmas[1] * init_loc_.relocalize_sigmas[1];
      const double syaw = init_loc_.relocalize_sigmas[2] * kDeg2Rad;
      cov[21] = syaw * syaw;
      relocalizeNearPose(fixed, cov);
    } else {
      seed_motion_model(this_obs_tim, fixed);
    }
    initial_localization_done_ = true;
  }
  // a pending relocalization request, served with a non-empty map, before the motion-model query
  const bool recovery = lost_.options().enabled;  // lost_recovery: (LidarOdometry.h)
  if (recovery) {
    rec.lost = lost_.lost();
    rec.bad_streak = lost_.badStreak();
  }
  if (reloc_request_ && !map_is_empty()) {
    if (recovery && lost_.ownPending()) {
      // the driver's own request: nobody could withdraw one that cannot be served, and it would throw on every scan from here on.
      // It is a failed attempt (rule 3 in LidarOdometry.h); the record shows the attempt and no search
      const auto t_served = std::chrono::steady_clock::now();
      try {
        serve_relocalization(this_obs_tim, rec);
      } catch (const std::runtime_error& e) {
        recovery_error_ = e.what();
        profile_["lost_recovery.not_served"] += 1.0;
        rec.relocalization_tried = rec.relocalized = rec.place_tried = false;
        rec.place_frames.clear(), rec.place_shifts.clear(), rec.place_dists.clear(), rec.reloc_ranks.clear();
        rec.reloc_candidates = rec.reloc_best_n_paired = 0;
        rec.reloc_best_quality = 0.0;
        note_served(rec, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_served).count());
      }
    } else {
      serve_relocalization(this_obs_tim, rec);
    }
  }

  bool updateLocalMap = false;
  bool map_trusted = true;  // lost_recovery: false while LOST -- the scan goes neither into the local maps nor into the key-frame store
  double kf_cov[36] = {0};  // the alignment's covariance, for the key-frame store (zeros for a first scan)
  {
    StageTimer tt(profile_, "onLidar.2.navstate");
    last_motion_model_output_ = navstate_.estimated_navstate(this_obs_tim);  // :810-811
  }
  const bool hasMotionModel = last_motion_model_output_.has_value();
  rec.had_motion_model = hasMotionModel;

  const bool map_empty = map_is_empty();
  if (map_empty) {
    // first point cloud: no ICP, it becomes the map (:817-838)
    rec.first_scan = true;
    updateLocalMap = true;
    trajectory_.emplace_back(this_obs_tim, last_lidar_pose_);
    navstate_.fuse_pose(this_obs_tim, CPose3D());
  } else {
    // ---- ICP (:840-1024)
    TPose3D init_guess = hasMotionModel ? last_motion_model_output_->pose.mean.asTPose() : last_lidar_pose_.asTPose();
    std::optional<CPose3DPDFGaussianInf> prior;
    if (hasMotionModel) {
      bool any = false;
      for (double v : last_motion_model_output_->pose.cov_inv) any = any || v != 0.0;
      if (any) prior = last_motion_model_output_->pose;
    }
    const int kind = hasMotionModel ? 0 : 1;
    const CPose3D last_keyframe_pose = last_lidar_pose_;
    double time_since_last_keyframe = 0;
    if (last_icp_timestamp_) time_since_last_keyframe = this_obs_tim - *last_icp_timestamp_;
    last_icp_timestamp_ = this_obs_tim;

    TPose3D current_solution = init_guess;
    rec.init_guess = CPose3D(init_guess);
    ICP& icp = *icp_[kind];
    StageTimer t_icp_all(profile_, "onLidar.3.icp_with_setup");
    mp2p_icp_hip::Parameters icp_params = icp_params_[kind];
    size_t remaining = icp_params.maxIterations;
    mp2p_icp_hip::Results res;
    mp2p_icp_hip::metric_map_t obs, glob;
    scan_layers(obs, glob);
    std::optional<StageTimer> t_icp;
    t_icp.emplace(profile_, "onLidar.3.run_icp");
    do {
      icp_params.maxIterations = (uint32_t)remaining;
      // the in-tree hook (:919-952) only compares the running solution with its check point: evaluated on the device.
      // NOTE the reference increments optimize_twist_max_corrections instead of its counter (:941), so the number of
      // corrections is bounded by the shared iteration budget only; kept.
      if (params_.optimize_twist)
        icp.setDeviceHook(params_.optimize_twist_rerun_min_trans, params_.optimize_twist_rerun_min_rot_deg * kDeg2Rad,
                          CPose3D(current_solution));
      else
        icp.clearHooks();
      icp.align(obs, glob, current_solution, icp_params, res, prior);  // :961-962
      rec.align_calls++;
      profile_["icp.host_polls"] += icp.lastAlignHostPolls();
      profile_["icp.enqueued_iterations"] += icp.lastAlignEnqueuedIterations();
      profile_["icp.executed_iterations"] += (double)res.nIterations;
      profile_["icp.align_calls"] += 1.0;
      if (gplan_) profile_["icp.fused_align_calls"] += icp.lastAlignUsedFusedPath() ? 1.0 : 0.0;  // (general plans: which route)
      profile_["onLidar.3.icp_host_setup"] += icp.lastAlignSetupSeconds();
      remaining -= std::min(remaining, res.nIterations);
      rec.icp_iterations += (uint32_t)res.nIterations;
      if (res.terminationReason == IterTermReason::HookRequest) {
        current_solution = res.optimal_tf.mean.asTPose();  // what the hook stored (:949)
        rec.twist_corrections++;
        if (time_since_last_keyframe > 0) {
          // re-estimate the twist from the running solution and de-skew again (:973-1004), all on the device
          const CPose3D incr = res.optimal_tf.mean - last_keyframe_pose;
          double w[3];
          incr.so3Log(w);
          const double At = time_since_last_keyframe;
          Twist tw;
          tw.vx = incr.T[3] / At; tw.vy = incr.T[7] / At; tw.vz = incr.T[11] / At;
          tw.wx = w[0] / At; tw.wy = w[1] / At; tw.wz = w[2] / At;
          updatePipelineTwistVariables(tw);
          source_.realize();
          if (!(gplan_ && gplan_->depth_input && !gplan_->has_2nd_pass)) run_second_pass();  // (no 2nd pass, no de-skew: nothing to run again)
          if (gplan_) record_layer_sizes(rec);  // (the record describes the layers that are aligned and merged in the end)
          rec.twist = tw;
        }
      }
    } while (res.terminationReason == IterTermReason::HookRequest);
    t_icp.reset();
    icp.clearHooks();
    rec.icp_run = true;
    rec.termination = (int)res.terminationReason;
    rec.goodness = res.quality;

    // ---- gate, motion model, trajectory (:1026-1045)
    StageTimer t_post(profile_, "onLidar.3.post_icp");
    const bool icpIsGood = res.quality >= params_.min_icp_goodness;
    last_icp_was_good_ = icpIsGood;
    last_icp_quality_ = res.quality;
    rec.icp_good = icpIsGood;
    if (params_.simplemap.generate) std::copy(&res.optimal_tf.cov[0], &res.optimal_tf.cov[0] + 36, kf_cov);
    if (icpIsGood) {
      last_lidar_pose_ = res.optimal_tf.mean;
      navstate_.fuse_pose(this_obs_tim, res.optimal_tf.mean, res.optimal_tf.cov);
      trajectory_.emplace_back(this_obs_tim, last_lidar_pose_);
    } else {
      navstate_.reset();
    }
    source_.updateVariable("icp_iterations", (double)res.nIterations);
    source_.updateVariable("twistCorrectionCount", 0);  // always 0 in the reference (App. C.2)

    // ---- adaptive threshold, also after a rejected ICP (:1052-1064)
    if (params_.adaptive_threshold_enabled) doUpdateAdaptiveThreshold(res.optimal_tf.mean - CPose3D(init_guess));

    // ---- lost_recovery: the streaks and the state follow the gate (a scan that restarts the map below stands outside them)
    if (recovery && !(!icpIsGood && trajectory_.size() == 1)) {
      const bool was_lost = lost_.lost();
      LostRecovery::Fields f;
      lost_.gate(icpIsGood, f);
      rec.bad_streak = f.bad_streak;
      if (!was_lost && lost_.lost()) lost_pose_ = last_lidar_pose_;  // (a rejected alignment has not moved it: the last good pose)
    }
    map_trusted = !recovery || !lost_.lost();

    // ---- key-frame decision (:1066-1118)
    const auto [isFirstPoseInChecker, distanceToClosest] = distance_checker_local_map_.check(last_lidar_pose_);
    const double dist_eucl_since_last = distanceToClosest.translationNorm();
    const double rot_since_last = distanceToClosest.rotationAngle();
    updateLocalMap = map_trusted && icpIsGood && params_.local_map_updates_enabled && hasMotionModel &&
                     (isFirstPoseInChecker || dist_eucl_since_last > params_.min_translation_between_keyframes ||
                      rot_since_last > params_.min_rotation_between_keyframes * kDeg2Rad);
    if (updateLocalMap) {
      distance_checker_local_map_.insert(last_lidar_pose_);
      if (params_.max_distance_to_keep_keyframes > 0 &&
          (localmap_check_removal_counter_++ >= params_.check_for_removal_every_n)) {
        localmap_check_removal_counter_ = 0;
        distance_checker_local_map_.removeAllFartherThan(last_lidar_pose_, params_.max_distance_to_keep_keyframes);
      }
    }
  }

  // a bad ICP right after the start: begin again from an empty map (:1146-1156)
  if (!last_icp_was_good_ && trajectory_.size() == 1) {
    resolve_map_counts();  // (earlier records keep the counts of the map they saw)
    if (local_map_) local_map_->clear();
    if (gplan_)
      for (auto& m : gplan_->maps)
        if (m.map && m.map != local_map_) m.map->clear();
    map_known_nonempty_ = false;
    map_points_cached_ = map_voxels_cached_ = 0;
    if (live_cleaner_) live_cleaner_->clear();  // (online_map_cleaning: whatever clears the maps empties the ring)
    trajectory_.clear();
    trajectory_anchor_.clear();
    updateLocalMap = false;
    last_icp_was_good_ = true;
    rec.restarted = true;
  }

  // ---- key-frames of the session (:1117-1138, 1209-1296), before the map update is queued: the download then waits for
  // nothing but this scan's own registration
  if (params_.simplemap.generate && !rec.restarted && map_trusted) store_keyframe(rec, rec.first_scan, rec.icp_good, kf_cov);

  // ---- local map update (:1158-1206): FilterMerge of the de-skewed map layer at the current pose, on the device
  if (updateLocalMap) {
    StageTimer tt(profile_, "onLidar.4.update_local_map");
    if (!local_map_) create_local_map();
    updatePipelineDynamicVariables();  // robot_x..robot_roll (:1194)
    resolve_map_counts();  // the previous update's counters (it finished before this scan's alignment started: no wait)
    // asynchronous: the update runs on the map's own stream and is waited for by the next use of the map only
    if (gplan_) {  // each FilterMerge into its own map, with that map's far-voxel removal
      for (const auto& [name, k] : gplan_->merges) {
        if (!gplan_->alive.count(name)) continue;
        const auto& m = gplan_->maps[k];
        m.map->insertPointCloud(*(name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name)),
                                last_lidar_pose_, m.remove_far);
      }
    } else {
      local_map_->insertPointCloud(*for_map_, last_lidar_pose_, remove_voxels_farther_than_);
    }
    rec.map_updated = true;
    if (live_opts_.enabled) rec.map_cleaned = clean_live_maps();  // online_map_cleaning: (LiveMapCleaning.h)
    if (rec.n_for_map == 0 || rec.map_cleaned) map_known_nonempty_ = false;  // (nothing offered, or points erased: ask the device next time)
    map_counts_pending_ = true;
    map_counts_from_ = records_.size() - 1;
  }
  // the next alignment's threshold schedules while the device works on the map update (the formulas' variables -- the
  // adaptive sigma -- are final for this scan; align() checks the values and evaluates again if they differ after all)
  if (icp_[0] && local_map_) icp_[0]->precomputeSchedule(icp_params_[0].maxIterations);
  if (params_.simplemap.generate && !kf_targets_known_ && local_map_) {  // (the maps exist from the first key-frame on)
    const auto targets = keyframe_targets();
    if (loaded_keyframes_.maps.empty()) kf_store_.setTargets(targets);
    else check_loaded_keyframe_targets(targets);  // (the file's header stays; the new frames must have been recorded for it)
    kf_targets_known_ = true;
  }
  if (loop_enabled_) feed_loop_closer(rec);
  if (recovery) {  // lost_recovery: the driver's own request, for the next observation to serve
    const uint32_t kind = lost_.due(reloc_request_.has_value(), !lost_.lost() || near_attempt_fits());
    if (kind) place_recovery_request(kind);
    rec.recovery_gave_up = lost_.gaveUp();
  }
  rec.pose = last_lidar_pose_;
  rec.sigma = adapt_thres_sigma_;
  rec.map_voxel_size = map_voxel_size_;
  if (!map_counts_pending_) {  // (otherwise filled by resolve_map_counts())
    rec.n_map_points = map_points_cached_;
    rec.n_map_voxels = map_voxels_cached_;
  }
  return rec;
}

// ---- online_map_cleaning: (LidarOdometry.h, LiveMapCleaning.h)
bool LidarOdometry::clean_live_maps() {
  if (!live_cleaner_) live_cleaner_ = std::make_unique<LiveMapCleaner>(live_opts_, ctx_);
  std::vector<HashedVoxelPointCloud*> targets;
  const auto wanted = [&](const std::string& name) {
    return live_opts_.target_maps.empty() || std::find(live_opts_.target_maps.begin(), live_opts_.target_maps.end(), name) != live_opts_.target_maps.end();
  };
  const DevicePointCloud* view = nullptr;
  if (gplan_) {
    for (const auto& m : gplan_->maps)
      if (m.map && wanted(m.name) && std::string(m.map->className()) != "CVoxelMap") targets.push_back(m.map.get());
    const std::string name = live_opts_.view_layer.empty() ? gplan_->merges.at(0).first : live_opts_.view_layer;
    if (!gplan_->alive.count(name))
      throw std::runtime_error("LidarOdometry (HIP): online_map_cleaning: view_layer '" + name + "' is not among the layers this scan's filters left");
    view = (name == "raw" ? (gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_) : gplan_->buf.at(name)).get();
  } else {
    targets.push_back(local_map_.get());
    view = (live_opts_.view_layer == plan_->layer_for_icp && live_opts_.view_layer != plan_->layer_for_map ? for_icp_ : for_map_).get();
  }
  return live_cleaner_->update(*view, last_lidar_pose_, targets);
}

uint64_t LidarOdometry::mapPointsErased() const {
  uint64_t total = 0;
  auto add = [&](const std::shared_ptr<HashedVoxelPointCloud>& m) {
    if (!m || std::string(m->className()) == "CVoxelMap") return;
    uint64_t n = 0;
    mp2p_icp_hip::check(mh_map_erased_total(m->handle(), &n), "mh_map_erased_total");
    total += n;
  };
  if (gplan_) for (const auto& m : gplan_->maps) add(m.map);
  else add(local_map_);
  return total;
}

// ---- gyro_deskew: (LidarOdometry.h, GyroDeskew.h)
void LidarOdometry::onGyro(double t, const double w[3]) {
  if (!gyro_opts_.enabled) return;  // (the block absent or disabled: nothing is kept, nothing is counted)
  gyro_buf_.push(t, w);
}

// ---- online_loop_closure: (LidarOdometry.h, LoopClosure.h)
CPose3D loop_raw_pose(const CPose3D& raw_prev, const CPose3D& P, const CPose3D& S_prev) {
  if (std::memcmp(raw_prev.T, S_prev.T, sizeof(raw_prev.T)) == 0) return P;  // nothing corrected yet: the raw chain IS the estimated one, bit for bit
  return raw_prev + (P - S_prev);
}
CPose3D loop_correction(const CPose3D& C, const CPose3D& P) { return C + (CPose3D() - P); }
CPose3D trajectory_anchor(const CPose3D& P, const CPose3D& S) { return P - S; }
CPose3D trajectory_corrected(const CPose3D& C, const CPose3D& rel) { return C + rel; }

void LidarOdometry::feed_loop_closer(ScanRecord& rec) {
  // every trajectory entry hangs on the last stored frame at or before it (this scan's own frame, when it was stored)
  const auto& stored = kf_store_.set().frames;
  while (trajectory_anchor_.size() < trajectory_.size()) {
    TrajectoryAnchor a;
    if (!stored.empty()) {
      a.frame = (long)stored.size() - 1;
      CPose3D S;
      std::copy(stored.back().pose, stored.back().pose + 12, S.T);
      a.rel = trajectory_anchor(trajectory_[trajectory_anchor_.size()].second, S);
    }
    trajectory_anchor_.push_back(a);
  }
  if (!kf_targets_known_ || loop_pushed_ >= stored.size()) return;
  StageTimer tt(profile_, "onLidar.6.loop_closure");
  if (!loop_closer_) {
    loop_closer_ = std::make_shared<OnlineLoopCloser>(kf_store_.set().maps, loop_cfg_, ctx_);
    loop_closer_->readFramesFrom(&stored);  // (the store's own layers: no second copy of the session's points)
  }
  bool closed = false;
  const size_t n_loaded = loaded_keyframes_.frames.size();
  for (; loop_pushed_ < stored.size(); loop_pushed_++) {
    const size_t k = loop_pushed_;
    CPose3D raw;  // raw_k = raw_{k-1} (+) (P_k (-) S_{k-1}); frame 0 and a loaded file's frames: their poses as they are
    std::copy(stored[k].pose, stored[k].pose + 12, raw.T);
    if (k > 0 && k >= n_loaded) {
      CPose3D S, R;
      std::copy(stored[k - 1].pose, stored[k - 1].pose + 12, S.T);
      std::copy(&loop_closer_->rawPoses()[12 * (k - 1)], &loop_closer_->rawPoses()[12 * (k - 1)] + 12, R.T);
      raw = loop_raw_pose(R, raw, S);
    }
    const OnlineLoopCloser::Step st = loop_closer_->pushStored(k, raw.T);
    const bool own = k + 1 == stored.size() && rec.simplemap_frame;  // this scan's frame
    if (own) {
      rec.loop_tried = st.tried;
      rec.loop_closed = st.closed;
      for (const auto& p : st.pairs) rec.loop_pairs.push_back(ScanRecord::LoopPairRecord{p.i, p.j, p.quality, p.accepted});
    }
    closed = closed || st.closed;
  }
  if (!loop_correct_ || loop_closer_->loops().empty()) return;
  // the store follows the closer: close_loops(rawKeyFrames()) gives keyFrames()' poses at any time
  CPose3D before;
  std::copy(stored.back().pose, stored.back().pose + 12, before.T);
  kf_store_.setPoses(loop_closer_->correctedPoses());
  if (closed) apply_loop_correction(rec, before);
}

void LidarOdometry::apply_loop_correction(ScanRecord& rec, const CPose3D& stored_pose_before) {
  StageTimer tt(profile_, "onLidar.6.loop_correction");  // (inside onLidar.6.loop_closure)
  const auto& set = kf_store_.set();
  CPose3D C;
  std::copy(set.frames.back().pose, set.frames.back().pose + 12, C.T);
  // ---- pose and motion model: delta = C_i (+) P_i^-1 moves the map frame
  CPose3D delta;
  if (rec.simplemap_frame) {  // the last stored frame is this scan's: its corrected pose is the vehicle's, bit for bit
    delta = loop_correction(C, last_lidar_pose_);
    last_lidar_pose_ = C;
  } else {  // (a closure among the frames of a loaded file, found at a scan that was not stored itself)
    delta = loop_correction(C, stored_pose_before);
    last_lidar_pose_ = delta + last_lidar_pose_;
  }
  navstate_.rebase(delta);
  if (last_motion_model_output_) last_motion_model_output_->pose.mean = delta + last_motion_model_output_->pose.mean;
  rec.loop_correction_trans = delta.translationNorm();
  rec.loop_correction_rot = delta.rotationAngle();
  // ---- local maps: cleared and rebuilt from the stored key-frames around the vehicle, one insertFrames per map
  resolve_map_counts();  // (earlier records keep the counts of the map they saw)
  auto rebuild = [&](HashedVoxelPointCloud& map, size_t k, bool first) {
    const double far = k < set.maps.size() ? (double)set.maps[k].remove_voxels_farther_than : 0.0;
    auto near = [&](const molahip_host::KeyFrame& f) {
      if (!(far > 0.0)) return true;
      const double dx = f.pose[3] - last_lidar_pose_.T[3], dy = f.pose[7] - last_lidar_pose_.T[7], dz = f.pose[11] - last_lidar_pose_.T[11];
      return std::sqrt(dx * dx + dy * dy + dz * dz) <= far;
    };
    map.clear();
    map.insertFrames(session_map_frames(set, k, near), 0);
    if (!first) return;
    // the local-map key-frame list becomes the poses of exactly the frames the first map was rebuilt from
    distance_checker_local_map_.clear();
    for (const auto& f : set.frames) {
      if (!f.has_points || !near(f)) continue;
      CPose3D p;
      std::copy(f.pose, f.pose + 12, p.T);
      distance_checker_local_map_.insert(p);
      rec.loop_rebuilt_frames++;
    }
  };
  if (gplan_) {
    for (size_t k = 0; k < gplan_->maps.size(); k++)
      if (gplan_->maps[k].map) rebuild(*gplan_->maps[k].map, k, k == 0);
  } else if (local_map_) {
    rebuild(*local_map_, 0, true);
  }
  map_known_nonempty_ = false;  // (ask the device)
  map_counts_pending_ = true;
  map_counts_from_ = records_.size() - 1;
}

molahip_host::KeyFrameSet LidarOdometry::rawKeyFrames() const {
  if (loop_closer_) return loop_closer_->rawKeyFrames();
  return molahip_host::KeyFrameSet();
}

std::vector<std::pair<double, CPose3D>> LidarOdometry::correctedTrajectory() const {
  std::vector<std::pair<double, CPose3D>> out = trajectory_;
  if (!loop_closer_ || loop_closer_->loops().empty()) return out;
  const std::vector<double>& C = loop_closer_->correctedPoses();
  for (size_t n = 0; n < out.size() && n < trajectory_anchor_.size(); n++) {
    const TrajectoryAnchor& a = trajectory_anchor_[n];
    if (a.frame < 0 || 12 * ((size_t)a.frame + 1) > C.size()) continue;
    CPose3D Ca;
    std::copy(&C[12 * (size_t)a.frame], &C[12 * (size_t)a.frame] + 12, Ca.T);
    out[n].second = trajectory_corrected(Ca, a.rel);
  }
  return out;
}

std::map<std::string, uint64_t> LidarOdometry::localMapSizes() const {
  std::map<std::string, uint64_t> sizes;
  if (gplan_) {
    for (const auto& m : gplan_->maps) sizes[m.name] = m.map ? m.map->size() : 0;
  } else if (plan_) {
    sizes[plan_->map_layer] = local_map_ ? local_map_->size() : 0;
  }
  return sizes;
}

std::map<std::string, LidarOdometry::MapStats> LidarOdometry::localMapStats() const {
  std::map<std::string, MapStats> out;
  auto stats = [](const std::shared_ptr<HashedVoxelPointCloud>& m, double voxel_size) {
    MapStats s;
    if (m) {
      s.n_points = m->size();  // (mh_map_get_info: waits for an update that still runs)
      s.n_voxels = m->voxelCount();
      s.voxel_size = voxel_size;
    }
    return s;
  };
  if (gplan_) {
    for (const auto& m : gplan_->maps) out[m.name] = stats(m.map, m.voxel_size);
  } else if (plan_) {
    out[plan_->map_layer] = stats(local_map_, map_voxel_size_);
  }
  return out;
}

std::map<std::string, std::string> LidarOdometry::localMapClasses() const {
  std::map<std::string, std::string> out;
  auto cls = [](const std::shared_ptr<HashedVoxelPointCloud>& m) -> std::string {
    if (!m) return "";
    if (std::dynamic_pointer_cast<mp2p_icp_hip::SparseTreesPointCloud>(m)) return "SparseTreesPointCloud";
    if (std::dynamic_pointer_cast<mp2p_icp_hip::CVoxelMap>(m)) return "CVoxelMap";
    return "HashedVoxelPointCloud";
  };
  if (gplan_) {
    for (const auto& m : gplan_->maps) out[m.name] = cls(m.map);
  } else if (plan_) {
    out[plan_->map_layer] = cls(local_map_);
  }
  return out;
}

LidarOdometry::LayerDump LidarOdometry::downloadLayer(const std::string& name) const {
  if (!gplan_) throw std::runtime_error("LidarOdometry::downloadLayer: only general plans keep their layers by name");
  std::shared_ptr<DevicePointCloud> l;
  if (name == "raw") {
    l = gplan_->raw_adjusted ? gplan_->raw_adjusted : cur_raw_;
  } else {
    const auto it = gplan_->buf.find(name);
    if (it != gplan_->buf.end()) l = it->second;
  }
  if (!l || name == kAdjustedRawKey) throw std::runtime_error("LidarOdometry::downloadLayer: no layer '" + name + "' in the last scan");
  LayerDump d;
  d.alive = gplan_->alive.count(name) != 0;
  const size_t n = l->size();
  d.x.resize(n); d.y.resize(n); d.z.resize(n); d.t.resize(n); d.src_idx.resize(n);
  if (!n) return d;
  check(mh_scan_download(l->handle(), d.x.data(), d.y.data(), d.z.data(), d.t.data(), d.src_idx.data()), "mh_scan_download");
  if (gplan_->reads_intensity) {  // ('raw' carries the channel, and every derived layer inherits it)
    d.intensity.resize(n);
    check(mh_scan_download_intensity(l->handle(), d.intensity.data()), "mh_scan_download_intensity");
  }
  return d;
}

LidarOdometry::MapDump LidarOdometry::downloadMap(const std::string& name) const {
  std::shared_ptr<HashedVoxelPointCloud> m;
  if (gplan_) {
    for (const auto& s : gplan_->maps)
      if (s.name == name) m = s.map;
  } else if (plan_ && plan_->map_layer == name) {
    m = local_map_;
  }
  MapDump d;
  if (!m) return d;  // (not created yet, or no such map: empty)
  // (the search structure's own counts: a CVoxelMap reports its occupied centres here, and its cells in downloadVoxelMap)
  mh_map_info mi{};
  check(mh_map_get_info(m->handle(), &mi), "mh_map_get_info");
  const size_t n = mi.n_points, v = mi.n_voxels;
  d.x.resize(n); d.y.resize(n); d.z.resize(n); d.src_idx.resize(n);
  d.vox_keys.resize(3 * v); d.vox_first.resize(v); d.vox_count.resize(v);
  if (!n) return d;
  check(mh_map_download(m->handle(), d.x.data(), d.y.data(), d.z.data(), d.src_idx.data(), d.vox_keys.data(), d.vox_first.data(),
                        d.vox_count.data()), "mh_map_download");
  return d;
}

LidarOdometry::VoxelMapDump LidarOdometry::downloadVoxelMap(const std::string& name) const {
  std::shared_ptr<HashedVoxelPointCloud> m;
  if (gplan_) {
    for (const auto& s : gplan_->maps)
      if (s.name == name) m = s.map;
  } else if (plan_ && plan_->map_layer == name) {
    m = local_map_;
  }
  VoxelMapDump d;
  if (!m) return d;  // (not created yet, or no such map: empty)
  auto vm = std::dynamic_pointer_cast<mp2p_icp_hip::CVoxelMap>(m);
  if (!vm) throw std::runtime_error("LidarOdometry::downloadVoxelMap: local map '" + name + "' is not a CVoxelMap");
  vm->download(d.keys, d.logodds);
  d.search_voxel_size = vm->searchVoxelSize();
  return d;
}

std::map<std::string, std::string> LidarOdometry::describePipeline() const {
  std::map<std::string, std::string> d;
  d["intensity_input"] = intensity_input_ ? "true" : "false";
  {
    char buf[96];
    snprintf(buf, sizeof(buf), "lidar_count %u max_time_offset %g", params_.lidar_count, params_.max_time_offset);
    d["multiple_lidars"] = buf;
    std::string labels;
    for (const auto& re : params_.lidar_sensor_labels) labels += (labels.empty() ? "" : " | ") + re;
    d["lidar_sensor_labels"] = params_.lidar_sensor_labels.empty() ? "(any)" : labels;
  }
  if (gplan_) {
    const GeneralPlan& g = *gplan_;
    d["plan"] = "general";
    d["input"] = g.depth_input ? "depth_image" : "point_cloud";
    d["timestamp_method"] = std::to_string(g.timestamp_method);
    size_t k = 0;
    for (const auto& st : g.steps) {
      std::string line = "pass" + std::to_string(st.pass) + " " + st.cls.substr(st.cls.rfind(':') == std::string::npos ? 0 : st.cls.rfind(':') + 1);
      if (st.kind == GeneralPlan::Kind::Delete) {
        line += " ";
        for (size_t i = 0; i < st.out.size(); i++) line += (i ? "," : "") + st.out[i];
      } else if (st.kind == GeneralPlan::Kind::EdgesFromRangeImage) {
        line += " depth image -> " + st.out[0] + "," + st.out[1] + " (row_window_length " + std::to_string(st.row_window_length) + ")";
      } else if (st.kind == GeneralPlan::Kind::NormalizeIntensity) {
        line += " " + st.in + " (in place" + (st.remember_range ? ", remembered range)" : ")");
      } else {
        line += " " + st.in + " ->";
        for (size_t i = 0; i < st.out.size(); i++) line += (i ? "," : " ") + (st.out[i].empty() ? std::string("-") : st.out[i]);
        if (st.bbox_mode != MH_BBOX_OFF) line += st.bbox_mode == MH_BBOX_KEEP_INSIDE ? " (inside)" : " (outside)";
      }
      char key[32];
      snprintf(key, sizeof(key), "step:%02zu", k++);
      d[key] = line;
    }
    d["steps"] = std::to_string(k);
    for (const auto& m : g.maps) d["map:" + m.name] = m.def["class"].asString();
    for (const auto& [layer, i] : g.merges) d["merge:" + layer] = g.maps[i].name;
    d["map_class"] = g.maps[0].def["class"].asString();
    d["icp_path"] = icp_[0] ? icp_[0]->alignPath() : "";
    for (const auto& p : g.declaredParameters()) d["formula:" + p.name + (d.count("formula:" + p.name) ? "#" + std::to_string(d.size()) : "")] = p.expr;
    for (const auto& p : params_.declaredParameters()) d["formula:" + p.name] = p.expr;
    return d;
  }
  if (!plan_) return d;
  d["layer_for_map"] = plan_->layer_for_map;
  d["layer_for_icp"] = plan_->layer_for_icp;
  d["map_layer"] = plan_->map_layer;
  d["map_class"] = map_def_["class"].asString();
  d["bbox_mode"] = std::to_string(plan_->bbox_mode);
  d["timestamp_method"] = std::to_string(plan_->timestamp_method);
  d["min_points_to_filter"] = std::to_string(plan_->min_points_to_filter);
  d["skip_deskew"] = plan_->skip_deskew ? "true" : "false";
  d["icp_path"] = icp_[0] ? icp_[0]->alignPath() : "";
  for (const auto& p : plan_->declaredParameters()) d["formula:" + p.name + (d.count("formula:" + p.name) ? "#" + std::to_string(d.size()) : "")] = p.expr;
  for (const auto& p : params_.declaredParameters()) d["formula:" + p.name] = p.expr;
  return d;
}

static void write_tum(const std::string& path, const std::vector<std::pair<double, CPose3D>>& trajectory) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("cannot write " + path);
  for (const auto& [t, p] : trajectory) {
    // rotation matrix -> unit quaternion (w >= 0)
    const double* T = p.T;
    const double tr = T[0] + T[5] + T[10];
    double qw, qx, qy, qz;
    if (tr > 0) {
      const double s = std::sqrt(tr + 1.0) * 2;
      qw = 0.25 * s; qx = (T[9] - T[6]) / s; qy = (T[2] - T[8]) / s; qz = (T[4] - T[1]) / s;
    } else if (T[0] > T[5] && T[0] > T[10]) {
      const double s = std::sqrt(1.0 + T[0] - T[5] - T[10]) * 2;
      qw = (T[9] - T[6]) / s; qx = 0.25 * s; qy = (T[1] + T[4]) / s; qz = (T[2] + T[8]) / s;
    } else if (T[5] > T[10]) {
      const double s = std::sqrt(1.0 + T[5] - T[0] - T[10]) * 2;
      qw = (T[2] - T[8]) / s; qx = (T[1] + T[4]) / s; qy = 0.25 * s; qz = (T[6] + T[9]) / s;
    } else {
      const double s = std::sqrt(1.0 + T[10] - T[0] - T[5]) * 2;
      qw = (T[4] - T[1]) / s; qx = (T[2] + T[8]) / s; qy = (T[6] + T[9]) / s; qz = 0.25 * s;
    }
    if (qw < 0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    fprintf(f, "%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", t, T[3], T[7], T[11], qx, qy, qz, qw);
  }
  fclose(f);
}

void LidarOdometry::saveTrajectoryTUM(const std::string& path) const { write_tum(path, trajectory_); }
void LidarOdometry::saveCorrectedTrajectoryTUM(const std::string& path) const { write_tum(path, correctedTrajectory()); }

}  // namespace mola_hip
