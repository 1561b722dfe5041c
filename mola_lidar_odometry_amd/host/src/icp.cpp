// icp.cpp -- mp2p_icp_hip: the reference's plugin classes re-stated as thin drivers of the C ABI.
// No arithmetic of the hot path happens here; see include/molahip.h for what each call replaces.
#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "mp2p_icp_hip/mp2p_icp_hip.h"
#include "molahip_host/hook_replay.h"
#include "molahip_host/layer_job_builder.h"
#include "molahip_host/plugin_switches.h"

namespace mp2p_icp_hip {

// ================================================================== poses (host-side glue only)
CPose3D::CPose3D(const TPose3D& p) {
  const double cy = cos(p.yaw), sy = sin(p.yaw), cp = cos(p.pitch), sp = sin(p.pitch), cr = cos(p.roll), sr = sin(p.roll);
  const double m[12] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, p.x,
                        sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, p.y,
                        -sp,     cp * sr,                cp * cr,                p.z};
  memcpy(T, m, sizeof(m));
}

TPose3D CPose3D::asTPose() const {
  TPose3D p;
  p.x = T[3]; p.y = T[7]; p.z = T[11];
  const double c = std::hypot(T[0], T[4]);
  p.pitch = atan2(-T[8], c);
  if (c > 1e-12) {
    p.yaw = atan2(T[4], T[0]);
    p.roll = atan2(T[9], T[10]);
  } else {
    p.yaw = atan2(-T[1], T[5]);
    p.roll = 0;
  }
  return p;
}

CPose3D CPose3D::operator+(const CPose3D& b) const {
  CPose3D c;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.T[i * 4 + j] = T[i * 4] * b.T[j] + T[i * 4 + 1] * b.T[4 + j] + T[i * 4 + 2] * b.T[8 + j];
    c.T[i * 4 + 3] = T[i * 4] * b.T[3] + T[i * 4 + 1] * b.T[7] + T[i * 4 + 2] * b.T[11] + T[i * 4 + 3];
  }
  return c;
}

CPose3D CPose3D::operator-(const CPose3D& b) const {  // b^-1 (+) a  (mrpt: a - b)
  CPose3D bi;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) bi.T[i * 4 + j] = b.T[j * 4 + i];
    bi.T[i * 4 + 3] = -(b.T[i] * b.T[3] + b.T[4 + i] * b.T[7] + b.T[8 + i] * b.T[11]);
  }
  return bi + *this;
}

double CPose3D::translationNorm() const { return std::sqrt(T[3] * T[3] + T[7] * T[7] + T[11] * T[11]); }

double CPose3D::rotationAngle() const {
  const double vx = T[9] - T[6], vy = T[2] - T[8], vz = T[4] - T[1];
  const double s2 = std::sqrt(vx * vx + vy * vy + vz * vz);
  double cth = 0.5 * (T[0] + T[5] + T[10] - 1.0);
  cth = std::min(1.0, std::max(-1.0, cth));
  return atan2(0.5 * s2, cth);
}

void CPose3D::so3Log(double w[3]) const {
  const double vx = T[9] - T[6], vy = T[2] - T[8], vz = T[4] - T[1];
  const double s2 = std::sqrt(vx * vx + vy * vy + vz * vz);  // 2 sin(th)
  const double th = rotationAngle();
  if (th < 1e-7) {
    const double k = 0.5 * (1.0 + th * th / 6.0);
    w[0] = k * vx; w[1] = k * vy; w[2] = k * vz;
    return;
  }
  if (M_PI - th > 1e-6) {
    const double k = th / s2;
    w[0] = k * vx; w[1] = k * vy; w[2] = k * vz;
    return;
  }
  // th ~ pi: R + I ~ 2 n n^T
  const double d[3] = {T[0], T[5], T[10]};
  const int k = (d[0] >= d[1] && d[0] >= d[2]) ? 0 : (d[1] >= d[2] ? 1 : 2);
  double n[3];
  const double nk = std::sqrt(std::max(0.0, 0.5 * (d[k] + 1.0)));
  for (int j = 0; j < 3; j++) n[j] = (j == k) ? nk : 0.25 * (T[k * 4 + j] + T[j * 4 + k]) / nk;
  const double dot = n[0] * vx + n[1] * vy + n[2] * vz;
  const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double sc = (dot < 0.0 ? -th : th) / nn;
  for (int j = 0; j < 3; j++) w[j] = sc * n[j];
}

CPose3D CPose3D::FromRotVecAndTranslation(const double w[3], const double t[3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
  double a, b;  // sin(th)/th, (1-cos th)/th^2
  if (th < 1e-2) {
    a = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0));
    b = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0));
  } else {
    const double sh = std::sin(0.5 * th);
    a = std::sin(th) / th;
    b = 2.0 * sh * sh / th2;
  }
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2], xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
  const double W2[9] = {-(yy + zz), xy, xz, xy, -(xx + zz), yz, xz, yz, -(xx + yy)};
  CPose3D p;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) p.T[i * 4 + j] = ((i == j) ? 1.0 : 0.0) + a * W[i * 3 + j] + b * W2[i * 3 + j];
    p.T[i * 4 + 3] = t[i];
  }
  return p;
}

// |v| and |w| of log_SE3(d) = [V^-1 t; w]  
static void se3_log_norms(const CPose3D& d, double& nt, double& nr) {
  const double* T = d.T;
  const double vx = T[9] - T[6], vy = T[2] - T[8], vz = T[4] - T[1];
  const double s2 = std::sqrt(vx * vx + vy * vy + vz * vz);
  const double th = d.rotationAngle();
  double w[3] = {0, 0, 0};
  if (s2 > 1e-300) {
    const double k = (th < 1e-7) ? 0.5 * (1.0 + th * th / 6.0) : th / s2;
    w[0] = k * vx; w[1] = k * vy; w[2] = k * vz;
  }
  const double th2 = th * th;
  const double kk = th < 1e-2 ? 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0 : (1.0 - 0.5 * th / std::tan(0.5 * th)) / th2;
  const double t[3] = {T[3], T[7], T[11]};
  // V^-1 t = t - 0.5 w x t + kk w x (w x t)
  const double c1[3] = {w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0]};
  const double c2[3] = {w[1] * c1[2] - w[2] * c1[1], w[2] * c1[0] - w[0] * c1[2], w[0] * c1[1] - w[1] * c1[0]};
  double v[3];
  for (int i = 0; i < 3; i++) v[i] = t[i] - 0.5 * c1[i] + kk * c2[i];
  nt = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  nr = th;
}

const char* enum2str(IterTermReason r) {
  static const char* n[] = {"Undefined", "NoPairings", "SolverError", "MaxIterations", "Stalled", "QualityCheckpointFailed",
                            "HookRequest"};
  return n[(int)r];
}

void throw_status(mh_status s, const char* where) {
  throw std::runtime_error(std::string(where) + ": " + mh_status_string(s) + ": " + mh_last_error_string());
}

// ================================================================== device handles
DeviceContext::DeviceContext(int device) : device_(device) { check(mh_ctx_create(device, nullptr, &ctx_), "mh_ctx_create"); }
void DeviceContext::synchronize() const { check(mh_ctx_synchronize(ctx_), "mh_ctx_synchronize"); }
DeviceContext::~DeviceContext() { mh_ctx_destroy(ctx_); }

std::shared_ptr<DeviceContext> DeviceContext::Default() {
  static std::mutex mtx;
  static std::weak_ptr<DeviceContext> weak;
  std::lock_guard<std::mutex> lk(mtx);
  auto sp = weak.lock();
  if (!sp) {
    sp = std::make_shared<DeviceContext>(0);
    weak = sp;
  }
  return sp;
}

HashedVoxelPointCloud::HashedVoxelPointCloud(float voxel_size, uint32_t max_points_per_voxel, std::shared_ptr<DeviceContext> ctx)
    : ctx_(std::move(ctx)) {
  mh_map_params p{};
  p.voxel_size = voxel_size;
  p.max_points_per_voxel = max_points_per_voxel;
  p.index_mode = molahip_host::plugin_switches().index_mode;          // MOLA_HIP_INDEX_MODE (default floor)
  p.far_voxel_metric = molahip_host::plugin_switches().far_voxel_metric;  // MOLA_HIP_FAR_VOXEL_METRIC (default Chebyshev)
  check(mh_map_create(ctx_->get(), &p, &map_), "mh_map_create");
  params_ = p;
}
HashedVoxelPointCloud::HashedVoxelPointCloud(const mh_map_params& p, std::shared_ptr<DeviceContext> ctx) : ctx_(std::move(ctx)) {
  check(mh_map_create(ctx_->get(), &p, &map_), "mh_map_create");
  params_ = p;
}

// ---- snapshot / restore
molahip_host::LocalMapRecord HashedVoxelPointCloud::snapshot(const std::string& name, float remove_voxels_farther_than) const {
  molahip_host::LocalMapRecord r;
  r.name = name;
  r.class_name = className();
  r.params = params_;
  r.remove_voxels_farther_than = remove_voxels_farther_than;
  mh_map_info mi{};
  check(mh_map_get_info(map_, &mi), "mh_map_get_info");
  r.n_offered = mi.n_offered;
  const size_t n = mi.n_points;
  r.x.resize(n); r.y.resize(n); r.z.resize(n); r.src_idx.resize(n);
  if (n) check(mh_map_download(map_, r.x.data(), r.y.data(), r.z.data(), r.src_idx.data(), nullptr, nullptr, nullptr), "mh_map_download");
  return r;
}
void HashedVoxelPointCloud::restore(const molahip_host::LocalMapRecord& rec) {
  if (rec.class_name != className())
    throw std::runtime_error(std::string("HashedVoxelPointCloud::restore: map '") + rec.name + "' was saved from a " + rec.class_name +
                             ", this object is a " + className());
  const mh_map_params &a = rec.params, &b = params_;
  if (a.voxel_size != b.voxel_size || a.max_points_per_voxel != b.max_points_per_voxel || a.index_mode != b.index_mode ||
      a.min_distance_between_points != b.min_distance_between_points || a.ndt_max_eigen_ratio != b.ndt_max_eigen_ratio ||
      a.ndt_min_points != b.ndt_min_points || a.far_voxel_metric != b.far_voxel_metric)
    throw std::runtime_error("HashedVoxelPointCloud::restore: map '" + rec.name + "' was saved with other parameters (voxel_size " +
                             std::to_string(a.voxel_size) + ", max_points_per_voxel " + std::to_string(a.max_points_per_voxel) +
                             ", index_mode " + std::to_string(a.index_mode) + ") than this map's (" + std::to_string(b.voxel_size) + ", " +
                             std::to_string(b.max_points_per_voxel) + ", " + std::to_string(b.index_mode) +
                             "); make_local_map() builds a map from the saved parameters");
  check(mh_map_restore(map_, rec.x.data(), rec.y.data(), rec.z.data(), rec.src_idx.data(), rec.x.size(), rec.n_offered, MH_MEM_HOST),
        "mh_map_restore");
}
void HashedVoxelPointCloud::saveToFile(const std::string& path, const std::string& name, float remove_voxels_farther_than) const {
  molahip_host::write_local_map_file(path, {snapshot(name, remove_voxels_farther_than)});
}
void HashedVoxelPointCloud::loadFromFile(const std::string& path, const std::string& name) {
  const std::vector<molahip_host::LocalMapRecord> maps = molahip_host::read_local_map_file(path);
  const molahip_host::LocalMapRecord* pick = nullptr;
  for (const auto& m : maps)
    if (name.empty() ? maps.size() == 1 : m.name == name) pick = &m;
  if (!pick)
    throw std::runtime_error("local map file '" + path + "': " + (name.empty() ? "holds " + std::to_string(maps.size()) + " maps: name the one to load"
                                                                                : "holds no map called '" + name + "'"));
  restore(*pick);
}
std::shared_ptr<HashedVoxelPointCloud> make_local_map(const molahip_host::LocalMapRecord& rec, std::shared_ptr<DeviceContext> ctx) {
  std::shared_ptr<HashedVoxelPointCloud> m;
  if (rec.class_name == "HashedVoxelPointCloud") m = std::make_shared<HashedVoxelPointCloud>(rec.params, std::move(ctx));
  else if (rec.class_name == "NDT") m = std::make_shared<NDT>(rec.params, std::move(ctx));
  else if (rec.class_name == "SparseTreesPointCloud") m = std::make_shared<SparseTreesPointCloud>(rec.params, std::move(ctx));
  else throw std::runtime_error("make_local_map: map '" + rec.name + "' is a '" + rec.class_name + "', which this loader cannot build");
  m->restore(rec);
  return m;
}
molahip_host::LocalMapRecord CVoxelMap::snapshot(const std::string&, float) const {
  throw std::runtime_error("CVoxelMap: an occupancy voxel map has no snapshot (saveToFile / saveLocalMaps cover HashedVoxelPointCloud, "
                           "NDT and SparseTreesPointCloud; the cells and log-odds of a CVoxelMap are not part of the map file yet)");
}
void CVoxelMap::restore(const molahip_host::LocalMapRecord&) {
  throw std::runtime_error("CVoxelMap: an occupancy voxel map cannot be restored from a map file (no snapshot of its cells and log-odds yet)");
}

static mh_map_params ndt_params(float vs, uint32_t cap, float min_dist, float ratio) {
  mh_map_params p{};
  p.voxel_size = vs;
  p.max_points_per_voxel = cap;
  p.index_mode = molahip_host::plugin_switches().index_mode;
  p.far_voxel_metric = molahip_host::plugin_switches().far_voxel_metric;
  p.min_distance_between_points = min_dist;
  p.ndt_max_eigen_ratio = ratio;
  p.ndt_min_points = 4;
  return p;
}
NDT::NDT(float voxel_size, uint32_t max_points_per_voxel, float min_distance_between_points, float max_eigen_ratio_for_planes,
         std::shared_ptr<DeviceContext> ctx)
    : HashedVoxelPointCloud(ndt_params(voxel_size, max_points_per_voxel, min_distance_between_points, max_eigen_ratio_for_planes),
                            std::move(ctx)) {}
size_t NDT::planeCount() const {
  mh_map_info i;
  check(mh_map_get_info(handle(), &i), "mh_map_get_info");
  return i.n_planes;
}
static mh_map_params sparse_trees_params(float grid_size, float minimum_points_clearance) {
  mh_map_params p{};
  p.voxel_size = grid_size;    // the cell
  p.max_points_per_voxel = 0;  // uncapped
  p.index_mode = molahip_host::plugin_switches().index_mode;
  p.far_voxel_metric = molahip_host::plugin_switches().far_voxel_metric;
  p.min_distance_between_points = minimum_points_clearance;
  return p;
}
SparseTreesPointCloud::SparseTreesPointCloud(float grid_size, float minimum_points_clearance, std::shared_ptr<DeviceContext> ctx)
    : HashedVoxelPointCloud(sparse_trees_params(grid_size, minimum_points_clearance), std::move(ctx)) {}
HashedVoxelPointCloud::~HashedVoxelPointCloud() { mh_map_destroy(map_); }

void HashedVoxelPointCloud::setPoints(const float* x, const float* y, const float* z, size_t n) {
  check(mh_map_build(map_, x, y, z, n, MH_MEM_HOST), "mh_map_build");
}

void HashedVoxelPointCloud::insertPoints(const float* x, const float* y, const float* z, size_t n) {
  // insertPoint for each point after everything already stored: the device-resident incremental update
  DevicePointCloud pc(ctx_);
  pc.setPoints(x, y, z, n);
  insertPointCloud(pc, CPose3D(), 0.f);
}

void HashedVoxelPointCloud::insertPointCloud(const DevicePointCloud& pc, const CPose3D& robot_pose,
                                             float remove_voxels_farther_than) {
  const mh_status st = mh_map_insert(map_, pc.handle(), robot_pose.T, remove_voxels_farther_than);
  if (st == MH_WARN_PREVIOUS_OUT_OF_RANGE) {  // this key-frame IS in the map; the one before it lost its wild points: log, go on
    fprintf(stderr, "[molahip] warning: %s\n", mh_last_error_string());
    return;
  }
  check(st, "mh_map_insert");
}

std::vector<mh_map_frame> to_map_frames(const std::vector<PosedFrame>& frames) {
  std::vector<mh_map_frame> f(frames.size());
  for (size_t k = 0; k < frames.size(); k++) {
    f[k].x = frames[k].x; f[k].y = frames[k].y; f[k].z = frames[k].z;
    f[k].n = frames[k].n;
    std::copy(frames[k].pose.T, frames[k].pose.T + 12, f[k].T);
  }
  return f;
}

void HashedVoxelPointCloud::insertFrames(const std::vector<PosedFrame>& frames, uint64_t max_points_per_pass) {
  const std::vector<mh_map_frame> f = to_map_frames(frames);
  const mh_status st = mh_map_insert_frames(map_, f.data(), f.size(), MH_MEM_HOST, max_points_per_pass);
  if (st == MH_WARN_PREVIOUS_OUT_OF_RANGE) {  // these frames ARE in the map; an earlier update lost its wild points: log, go on
    fprintf(stderr, "[molahip] warning: %s\n", mh_last_error_string());
    return;
  }
  check(st, "mh_map_insert_frames");
}

void HashedVoxelPointCloud::clear() { check(mh_map_build(map_, nullptr, nullptr, nullptr, 0, MH_MEM_HOST), "mh_map_build"); }

RadiusResults HashedVoxelPointCloud::radiusSearch(const DevicePointCloud& queries, const CPose3D& T, double radius, bool sorted) const {
  prepareSearch(radius);
  RadiusResults r;
  const size_t n = queries.size();
  r.offsets.assign(n + 1, 0u);
  const uint32_t flags = sorted ? MH_RADIUS_SORTED : MH_RADIUS_VISIT_ORDER;
  mh_radius_out out{};
  mh_radius_info info{};
  out.offsets = r.offsets.data();
  check(mh_nn_search_radius(map_, queries.handle(), T.T, radius, flags, &out, MH_MEM_HOST, &info), "mh_nn_search_radius");
  r.maxPerQuery = info.max_per_query;
  const size_t k = (size_t)info.n_results;
  if (!k) return r;
  r.globalIdx.resize(k);
  r.gx.resize(k); r.gy.resize(k); r.gz.resize(k); r.errSq.resize(k);
  out.global_idx = r.globalIdx.data();
  out.gx = r.gx.data(); out.gy = r.gy.data(); out.gz = r.gz.data(); out.d2 = r.errSq.data();
  out.capacity = k;
  check(mh_nn_search_radius(map_, queries.handle(), T.T, radius, flags, &out, MH_MEM_HOST, &info), "mh_nn_search_radius");
  if (info.n_written != k) throw std::runtime_error("mh_nn_search_radius: the map changed between the counting and the sized call");
  return r;
}
RadiusResults HashedVoxelPointCloud::radiusSearch(const float* x, const float* y, const float* z, size_t n, const CPose3D& T,
                                                  double radius, bool sorted) const {
  DevicePointCloud pc(ctx_);
  pc.setPoints(x, y, z, n);
  return radiusSearch(pc, T, radius, sorted);
}

DevicePointCloud::DevicePointCloud(std::shared_ptr<DeviceContext> ctx) : ctx_(std::move(ctx)) {
  check(mh_scan_create(ctx_->get(), nullptr, nullptr, nullptr, 0, MH_MEM_HOST, &scan_), "mh_scan_create");
}
DevicePointCloud::~DevicePointCloud() { mh_scan_destroy(scan_); }
size_t DevicePointCloud::size() const {
  uint64_t n = 0;
  check(mh_scan_size(scan_, &n), "mh_scan_size");
  return n;
}
void DevicePointCloud::setPoints(const float* x, const float* y, const float* z, size_t n) {
  check(mh_scan_update(scan_, x, y, z, n, MH_MEM_HOST), "mh_scan_update");
}
void DevicePointCloud::setPointsInterleaved(const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y,
                                            size_t off_z, long long off_t, bool pinned, long long off_i) {
  check(mh_scan_update_aos_i(scan_, data, n, point_step, off_x, off_y, off_z, (int64_t)off_t, (int64_t)off_i,
                             pinned ? MH_MEM_HOST_PINNED : MH_MEM_HOST),
        "mh_scan_update_aos_i");
}
void DevicePointCloud::setIntensity(const float* i, size_t n) {
  check(mh_scan_set_intensity(scan_, i, n, MH_MEM_HOST), "mh_scan_set_intensity");
}
void DevicePointCloud::setTimestamps(const float* t, size_t n) {
  check(mh_scan_set_timestamps(scan_, t, n, MH_MEM_HOST), "mh_scan_set_timestamps");
}
void DevicePointCloud::boundingBox(float mn[3], float mx[3]) const {
  check(mh_scan_bbox(scan_, mn, mx, nullptr), "mh_scan_bbox");
}
void DevicePointCloud::download(std::vector<float>& x, std::vector<float>& y, std::vector<float>& z) const {
  const size_t n = size();
  x.resize(n); y.resize(n); z.resize(n);
  check(mh_scan_download(scan_, x.data(), y.data(), z.data(), nullptr, nullptr), "mh_scan_download");
}

size_t HashedVoxelPointCloud::size() const {
  mh_map_info i;
  check(mh_map_get_info(map_, &i), "mh_map_get_info");
  return i.n_points;
}
size_t HashedVoxelPointCloud::voxelCount() const {
  mh_map_info i;
  check(mh_map_get_info(map_, &i), "mh_map_get_info");
  return i.n_voxels;
}

// ---- CVoxelMap
mh_occmap_params CVoxelMap::defaultParams(float resolution) {
  mh_occmap_params p{};
  p.resolution = resolution;
  p.prob_hit = 0.70f;
  p.prob_miss = 0.30f;
  p.clamp_min = 0.05f;
  p.clamp_max = 0.95f;
  p.occupied_threshold = 0.60f;
  p.ray_trace_free_space = 1;
  p.decimation = 1;
  p.update_rule = molahip_host::plugin_switches().voxelmap_update;    // MOLA_HIP_VOXELMAP_UPDATE (default counted)
  p.index_mode = molahip_host::plugin_switches().index_mode;          // MOLA_HIP_INDEX_MODE
  p.far_voxel_metric = molahip_host::plugin_switches().far_voxel_metric;  // MOLA_HIP_FAR_VOXEL_METRIC
  return p;
}
CVoxelMap::CVoxelMap(const mh_occmap_params& p, std::shared_ptr<DeviceContext> ctx) : HashedVoxelPointCloud(NoMap{}, std::move(ctx)) {
  check(mh_occmap_create(ctx_->get(), &p, &occ_), "mh_occmap_create");
  prepareSearch(0.0);
}
CVoxelMap::~CVoxelMap() {
  mh_occmap_destroy(occ_);
  map_ = nullptr;  // (the search map was the occupancy map's own)
}
void CVoxelMap::setPoints(const float*, const float*, const float*, size_t) {
  throw std::runtime_error("CVoxelMap::setPoints: an occupancy map is updated by insertPointCloud (ray tracing from a pose)");
}
void CVoxelMap::insertPoints(const float*, const float*, const float*, size_t) {
  throw std::runtime_error("CVoxelMap::insertPoints: an occupancy map is updated by insertPointCloud (ray tracing from a pose)");
}
float CVoxelMap::searchVoxelSize() const {
  mh_occmap_info i;
  check(mh_occmap_get_info(occ_, &i), "mh_occmap_get_info");
  return i.search_voxel_size;
}
void CVoxelMap::insertPointCloud(const DevicePointCloud& pc, const CPose3D& robot_pose, float remove_voxels_farther_than) {
  check(mh_occmap_insert(occ_, pc.handle(), robot_pose.T, remove_voxels_farther_than), "mh_occmap_insert");
  prepareSearch(0.0);
}
void CVoxelMap::insertFrames(const std::vector<PosedFrame>&, uint64_t) {
  throw std::runtime_error("CVoxelMap::insertFrames: an occupancy map is updated by ray tracing from the pose each scan was seen from "
                           "(insertPointCloud), not by inserting point layers; it has no batched insertion");
}
void CVoxelMap::insertPointCloudFrames(const std::vector<PosedFrame>& frames, uint64_t max_points_per_pass) {
  const std::vector<mh_map_frame> f = to_map_frames(frames);
  const mh_status st = mh_occmap_insert_frames(occ_, f.data(), f.size(), MH_MEM_HOST, max_points_per_pass);
  prepareSearch(0.0);  // (a failed call may have applied earlier passes: the search map is the occupancy map's present one)
  check(st, "mh_occmap_insert_frames");
}
bool CVoxelMap::indexBounds(int32_t lo[3], int32_t hi[3]) const {
  uint64_t n = 0;
  check(mh_occmap_index_bounds(occ_, lo, hi, &n), "mh_occmap_index_bounds");
  return n > 0;
}
std::vector<int32_t> CVoxelMap::projectGrid(const mh_occgrid_window& window) const {
  std::vector<int32_t> out((size_t)window.nx * window.ny);
  check(mh_occmap_project_grid(occ_, &window, out.data()), "mh_occmap_project_grid");
  return out;
}
mh_occmap_info CVoxelMap::occInfo() const {
  mh_occmap_info i;
  check(mh_occmap_get_info(occ_, &i), "mh_occmap_get_info");
  return i;
}
void CVoxelMap::clear() {
  check(mh_occmap_clear(occ_), "mh_occmap_clear");
  prepareSearch(0.0);
}
size_t CVoxelMap::size() const {
  mh_occmap_info i;
  check(mh_occmap_get_info(occ_, &i), "mh_occmap_get_info");
  return i.n_occupied;
}
size_t CVoxelMap::voxelCount() const {
  mh_occmap_info i;
  check(mh_occmap_get_info(occ_, &i), "mh_occmap_get_info");
  return i.n_cells;
}
void CVoxelMap::prepareSearch(double max_radius) const {
  const mh_map* m = nullptr;
  map_ = nullptr;  // (a growing call replaces the search map: nothing of the old one is kept across it, whatever it returns)
  check(mh_occmap_search_map(occ_, (float)max_radius, &m), "mh_occmap_search_map");
  map_ = const_cast<mh_map*>(m);  // (the entry points that take it read it only)
}
void CVoxelMap::download(std::vector<int32_t>& keys_xyz, std::vector<int32_t>& logodds) const {
  const size_t n = voxelCount();
  keys_xyz.resize(3 * n);
  logodds.resize(n);
  if (n) check(mh_occmap_download(occ_, keys_xyz.data(), logodds.data()), "mh_occmap_download");
}

// ================================================================== parameters
static uint32_t to_u32(const std::string& s) { return (uint32_t)strtoul(s.c_str(), nullptr, 10); }
static bool to_bool(const std::string& s) { return s == "true" || s == "True" || s == "1" || s == "yes"; }

void Parameters::load_from(const Config& c) {
  if (c.has("maxIterations")) maxIterations = to_u32(c["maxIterations"].asString());
  if (c.has("minAbsStep_trans")) minAbsStep_trans = strtod(c["minAbsStep_trans"].asString().c_str(), nullptr);
  if (c.has("minAbsStep_rot")) minAbsStep_rot = strtod(c["minAbsStep_rot"].asString().c_str(), nullptr);
  if (c.has("generateDebugFiles")) generateDebugFiles = to_bool(c["generateDebugFiles"].asString());
  if (c.has("debugFileNameFormat")) {
    debugFileNameFormat = c["debugFileNameFormat"].asString();
    const std::string ext = ".icplog";  // the JSON trace must not masquerade as an MRPT-serialised .icplog
    if (debugFileNameFormat.size() >= ext.size() && debugFileNameFormat.compare(debugFileNameFormat.size() - ext.size(), ext.size(), ext) == 0)
      debugFileNameFormat += ".json";
  }
}

// ================================================================== matcher
bool Matcher::match(const metric_map_t& pcGlobal, const metric_map_t& pcLocal, const CPose3D& localPose,
                    const MatchContext& mc, Pairings& out) const {
  if (!enabled) return false;
  if (runFromIteration != 0 && mc.icpIteration < runFromIteration) return false;
  if (runUpToIteration != 0 && mc.icpIteration > runUpToIteration) return false;
  impl_match(pcGlobal, pcLocal, localPose, mc, out);
  return true;
}

void Matcher_Points_DistanceThreshold::initialize(const Config& c) {
  parameterFromConfig(c, "threshold", &threshold, true);
  parameterFromConfig(c, "thresholdAngularDeg", &thresholdAngularDeg, false);
  if (c.has("pairingsPerPoint")) pairingsPerPoint = to_u32(c["pairingsPerPoint"].asString());
  if (c.has("allowMatchAlreadyMatchedGlobalPoints"))
    allowMatchAlreadyMatchedGlobalPoints = to_bool(c["allowMatchAlreadyMatchedGlobalPoints"].asString());
  if (c.has("runFromIteration")) runFromIteration = to_u32(c["runFromIteration"].asString());
  if (c.has("runUpToIteration")) runUpToIteration = to_u32(c["runUpToIteration"].asString());
  pointLayerMatches.clear();
  if (c.has("pointLayerMatches")) {
    const Config& s = c["pointLayerMatches"];
    for (size_t i = 0; i < s.size(); i++) {
      LayerMatch lm;
      lm.global = s.at(i)["global"].asString();
      lm.local = s.at(i)["local"].asString();
      lm.weight = strtod(s.at(i).getOr("weight", "1.0").c_str(), nullptr);
      pointLayerMatches.push_back(lm);
    }
  }
  if (pairingsPerPoint < 1 || pairingsPerPoint > MH_MAX_PAIRINGS_PER_POINT)
    throw std::runtime_error("Matcher_Points_DistanceThreshold: pairingsPerPoint must be 1.." +
                             std::to_string(MH_MAX_PAIRINGS_PER_POINT) + " (rgbd.yaml:138 uses 2)");
}

static const PointCloud& local_layer(const metric_map_t& m, const std::string& name) {
  auto it = m.layers.find(name);
  if (it == m.layers.end()) throw std::runtime_error("local layer '" + name + "' not found");
  auto p = std::dynamic_pointer_cast<PointCloud>(it->second);
  if (!p) throw std::runtime_error("local layer '" + name + "' is not a point cloud");
  return *p;
}
// ... for the matcher-granular loop, which reads the local points on the host: a device-resident layer (the stand-alone driver's
// general plans hand over DevicePointCloud) is downloaded into `downloaded` first
static const PointCloud& local_layer(const metric_map_t& m, const std::string& name, PointCloud& downloaded) {
  auto it = m.layers.find(name);
  if (it != m.layers.end())
    if (auto dev = std::dynamic_pointer_cast<DevicePointCloud>(it->second)) {
      dev->download(downloaded.x, downloaded.y, downloaded.z);
      return downloaded;
    }
  return local_layer(m, name);
}
static const HashedVoxelPointCloud& global_layer(const metric_map_t& m, const std::string& name) {
  auto it = m.layers.find(name);
  if (it == m.layers.end()) throw std::runtime_error("global layer '" + name + "' not found");
  auto p = std::dynamic_pointer_cast<HashedVoxelPointCloud>(it->second);
  if (!p) throw std::runtime_error("global layer '" + name + "' is not NearestNeighborsCapable on the device");
  return *p;
}

void Matcher_Points_DistanceThreshold::impl_match(const metric_map_t& pcGlobal, const metric_map_t& pcLocal,
                                                  const CPose3D& localPose, const MatchContext&, Pairings& out) const {
  for (const auto& lm : pointLayerMatches) {
    PointCloud downloaded;
    const PointCloud& loc = local_layer(pcLocal, lm.local, downloaded);
    const HashedVoxelPointCloud& glob = global_layer(pcGlobal, lm.global);
    const size_t n = loc.size();
    out.potential_pairings += n * pairingsPerPoint;
    // (the fused multi-layer path, ICP::align_fused_layers, takes a weight per pair; this matcher-granular path keeps its refusal)
    if (out.pt2pt_weight_set && out.pt2pt_weight != lm.weight)
      throw std::runtime_error("pointLayerMatches with different weights in one pairing set: not a device input (one weight per kind of pair)");
    out.pt2pt_weight = lm.weight;
    out.pt2pt_weight_set = true;
    if (!n) continue;
    mh_scan* scan = nullptr;
    check(mh_scan_create(glob.context()->get(), loc.x.data(), loc.y.data(), loc.z.data(), n, MH_MEM_HOST, &scan), "mh_scan_create");
    const size_t cap = n * pairingsPerPoint;  // nn_multiple_search(k): up to k pairs per local point (rgbd.yaml:138)
    std::vector<uint32_t> li(cap), gi(cap);
    std::vector<float> gx(cap), gy(cap), gz(cap), d2(cap);
    mh_pairs_out po{li.data(), gi.data(), gx.data(), gy.data(), gz.data(), d2.data()};
    mh_match_info info{};
    glob.prepareSearch(threshold);
    const mh_status st = mh_nn_search_k(glob.handle(), scan, localPose.T, threshold, thresholdAngularDeg, pairingsPerPoint, &po,
                                        MH_MEM_HOST, &info);
    mh_scan_destroy(scan);
    check(st, "mh_nn_search_k");
    // U12 (MOLA_HIP_MATCHED_POINTS=skip): local points an earlier matcher of this iteration has paired are left out [U]
    const bool skip_paired = molahip_host::plugin_switches().matched_points == MH_MATCHED_POINTS_SKIP;
    auto& paired = out.local_paired[lm.local];
    if (paired.size() < n) paired.resize(n, 0);
    std::vector<uint8_t> paired_before;
    if (skip_paired) paired_before = paired;  // (a point's own second pair is not "already paired by an earlier matcher")
    // U13 (allowMatchAlreadyMatchedGlobalPoints: false): the pairs arrive in ascending local index, so this is upstream's serial
    // walk [U] -- a candidate whose map point an earlier candidate of this iteration has taken is dropped, every other one takes
    // its map point; with pairingsPerPoint > 1 each of a point's candidates on its own
    const bool unique = !allowMatchAlreadyMatchedGlobalPoints;
    std::vector<uint8_t>* const claimed = unique ? &out.global_paired[lm.global] : nullptr;
    for (size_t k = 0; k < info.n_pairs; k++) {
      if (skip_paired && paired_before[li[k]]) continue;
      if (unique) {
        if (claimed->size() <= gi[k]) claimed->resize((size_t)gi[k] + 1, 0);
        if ((*claimed)[gi[k]]) continue;
        (*claimed)[gi[k]] = 1;
      }
      paired[li[k]] = 1;
      out.localIdx.push_back(li[k]);
      out.globalIdx.push_back(gi[k]);
      out.lx.push_back(loc.x[li[k]]);
      out.ly.push_back(loc.y[li[k]]);
      out.lz.push_back(loc.z[li[k]]);
      out.gx.push_back(gx[k]);
      out.gy.push_back(gy[k]);
      out.gz.push_back(gz[k]);
      out.errSq.push_back(d2[k]);
    }
  }
}

void Matcher_Point2Plane::initialize(const Config& c) {
  parameterFromConfig(c, "distanceThreshold", &distanceThreshold, true);
  parameterFromConfig(c, "planeEigenThreshold", &planeEigenThreshold, false);
  parameterFromConfig(c, "searchRadius", &searchRadius, false);
  if (c.has("knn")) knn = to_u32(c["knn"].asString());
  if (c.has("minimumPlanePoints")) minimumPlanePoints = to_u32(c["minimumPlanePoints"].asString());
  // (kept for the pipelines that write it; never applied -- plane pairings name no map point, so there is nothing to claim, U13)
  if (c.has("allowMatchAlreadyMatchedGlobalPoints"))
    allowMatchAlreadyMatchedGlobalPoints = to_bool(c["allowMatchAlreadyMatchedGlobalPoints"].asString());
  if (c.has("runFromIteration")) runFromIteration = to_u32(c["runFromIteration"].asString());
  if (c.has("runUpToIteration")) runUpToIteration = to_u32(c["runUpToIteration"].asString());
  pointLayerMatches.clear();
  if (c.has("pointLayerMatches")) {
    const Config& s = c["pointLayerMatches"];
    for (size_t i = 0; i < s.size(); i++) {
      Matcher_Points_DistanceThreshold::LayerMatch lm;
      lm.global = s.at(i)["global"].asString();
      lm.local = s.at(i)["local"].asString();
      lm.weight = strtod(s.at(i).getOr("weight", "1.0").c_str(), nullptr);
      pointLayerMatches.push_back(lm);
    }
  }
}

static void append_pl_pairs(const PointCloud& loc, const std::vector<uint32_t>& li, const std::vector<float>* a, size_t k,
                            Pairings& out) {
  for (size_t i = 0; i < k; i++) {
    out.pl_lx.push_back(loc.x[li[i]]);
    out.pl_ly.push_back(loc.y[li[i]]);
    out.pl_lz.push_back(loc.z[li[i]]);
    out.pl_cx.push_back(a[0][i]);
    out.pl_cy.push_back(a[1][i]);
    out.pl_cz.push_back(a[2][i]);
    out.pl_nx.push_back(a[3][i]);
    out.pl_ny.push_back(a[4][i]);
    out.pl_nz.push_back(a[5][i]);
  }
}

void Matcher_Point2Plane::impl_match(const metric_map_t& pcGlobal, const metric_map_t& pcLocal, const CPose3D& localPose,
                                     const MatchContext&, Pairings& out) const {
  for (const auto& lm : pointLayerMatches) {
    const PointCloud& loc = local_layer(pcLocal, lm.local);
    const HashedVoxelPointCloud& glob = global_layer(pcGlobal, lm.global);
    const size_t n = loc.size();
    out.potential_pairings += n;
    if (out.pt2pl_weight_set && out.pt2pl_weight != lm.weight)
      throw std::runtime_error("Matcher_Point2Plane layers with different weights in one pairing set: not a device input");
    out.pt2pl_weight = lm.weight;  // [U] whether upstream applies a layer weight to plane pairs is unverified; every shipped pipeline has 1.0
    out.pt2pl_weight_set = true;
    if (!n) continue;
    mh_scan* scan = nullptr;
    check(mh_scan_create(glob.context()->get(), loc.x.data(), loc.y.data(), loc.z.data(), n, MH_MEM_HOST, &scan), "mh_scan_create");
    std::vector<uint32_t> li(n);
    std::vector<float> a[6];
    for (auto& v : a) v.resize(n);
    mh_pairs_pl_out po{li.data(), a[0].data(), a[1].data(), a[2].data(), a[3].data(), a[4].data(), a[5].data()};
    mh_match_info info{};
    mh_status st;
    glob.prepareSearch(std::max(distanceThreshold, searchRadius));
    if (dynamic_cast<const NDT*>(&glob)) {  // per-voxel planes
      st = mh_nn_search_pt2pl(glob.handle(), scan, localPose.T, distanceThreshold, molahip_host::plugin_switches().pt2pl_mode, &po,
                              MH_MEM_HOST, &info);
    } else {  // a plain point layer: k nearest neighbours + PCA (rgbd.yaml:143-151)
      mh_pt2pl_knn_params kp{distanceThreshold, planeEigenThreshold, searchRadius, knn, minimumPlanePoints};
      st = mh_nn_search_pt2pl_knn(glob.handle(), scan, localPose.T, &kp, &po, MH_MEM_HOST, &info);
    }
    mh_scan_destroy(scan);
    check(st, "mh_nn_search_pt2pl");
    append_pl_pairs(loc, li, a, info.n_pairs, out);
    auto& paired = out.local_paired[lm.local];  // (what MatchState::localPairedBitField records upstream [U])
    if (paired.size() < n) paired.resize(n, 0);
    for (size_t k = 0; k < info.n_pairs; k++) paired[li[k]] = 1;
  }
}

// ================================================================== solver
static RobustKernel parse_kernel(std::string s) {
  const size_t p = s.rfind("::");
  if (p != std::string::npos) s = s.substr(p + 2);
  if (s == "None") return RobustKernel::None;
  if (s == "GemanMcClure") return RobustKernel::GemanMcClure;
  if (s == "Cauchy") return RobustKernel::Cauchy;
  if (s == "GemanMcClure_KISS") return RobustKernel::GemanMcClure_KISS;
  if (s == "GemanMcClure_Barron") return RobustKernel::GemanMcClure_Barron;
  if (s == "GemanMcClure_C2") return RobustKernel::GemanMcClure_C2;
  throw std::runtime_error("unknown robustKernel '" + s + "'");
}

void Solver_GaussNewton::initialize(const Config& c) {
  if (c.has("maxIterations")) maxIterations = to_u32(c["maxIterations"].asString());
  if (c.has("robustKernel")) robustKernel = parse_kernel(c["robustKernel"].asString());
  parameterFromConfig(c, "robustKernelParam", &robustKernelParam, false);
  if (c.has("minDelta")) minDelta = strtod(c["minDelta"].asString().c_str(), nullptr);
  if (c.has("maxCost")) maxCost = strtod(c["maxCost"].asString().c_str(), nullptr);
}

static mh_gn_params gn_params_of(const Solver_GaussNewton& s) {
  mh_gn_params p{};
  p.max_inner_iterations = s.maxIterations;
  p.robust_kernel = (uint32_t)s.robustKernel;
  p.robust_kernel_param = s.robustKernelParam;
  p.min_delta = s.minDelta;
  p.max_cost = s.maxCost;
  p.weight_pt2pt = 1.0;
  p.weight_pt2pl = 1.0;
  return p;
}

static void fill_prior(const std::optional<CPose3DPDFGaussianInf>& prior, mh_prior& out) {
  memcpy(out.mean, prior->mean.T, sizeof(out.mean));
  memcpy(out.info, prior->cov_inv, sizeof(out.info));
}

bool Solver_GaussNewton::optimal_pose(const Pairings& p, OptimalTF_Result& out, const SolverContext& sc) const {
  if (!sc.guessRelativePose) throw std::runtime_error("Solver_GaussNewton: guessRelativePose is required");
  mh_pairs_pt2pt pp{p.lx.data(), p.ly.data(), p.lz.data(), p.gx.data(), p.gy.data(), p.gz.data(), p.localIdx.size()};
  mh_pairs_pt2pl pl{p.pl_lx.data(), p.pl_ly.data(), p.pl_lz.data(), p.pl_cx.data(), p.pl_cy.data(), p.pl_cz.data(),
                    p.pl_nx.data(), p.pl_ny.data(), p.pl_nz.data(), p.pl_lx.size()};
  mh_gn_params gp = gn_params_of(*this);
  gp.weight_pt2pt = p.pt2pt_weight;  // the layer weight of the matcher that produced the pairs (Pairings::point_weights [U])
  gp.weight_pt2pl = p.pt2pl_weight;
  mh_prior pr;
  if (sc.prior) fill_prior(sc.prior, pr);
  double T[12];
  memcpy(T, sc.guessRelativePose->T, sizeof(T));
  int32_t n_steps = 0, ok = 1;
  check(mh_gn_solve(DeviceContext::Default()->get(), &pp, &pl, MH_MEM_HOST, &gp, sc.prior ? &pr : nullptr, T, &n_steps, &ok, nullptr),
        "mh_gn_solve");
  memcpy(out.optimalPose.T, T, sizeof(T));
  return ok != 0;
}

// ================================================================== factory
Matcher::Ptr create_matcher(const std::string& cn) {
  if (cn == "mp2p_icp::Matcher_Points_DistanceThreshold" || cn == "mp2p_icp_hip::Matcher_Points_DistanceThreshold")
    return std::make_shared<Matcher_Points_DistanceThreshold>();
  if (cn == "mp2p_icp::Matcher_Point2Plane" || cn == "mp2p_icp_hip::Matcher_Point2Plane")
    return std::make_shared<Matcher_Point2Plane>();
  throw std::runtime_error("matcher class '" + cn + "' is not available in mp2p_icp_hip");
}
Solver::Ptr create_solver(const std::string& cn) {
  if (cn == "mp2p_icp::Solver_GaussNewton" || cn == "mp2p_icp_hip::Solver_GaussNewton")
    return std::make_shared<Solver_GaussNewton>();
  throw std::runtime_error("solver class '" + cn + "' is not available in mp2p_icp_hip");
}

// ================================================================== ICP
ICP::ICP(std::shared_ptr<DeviceContext> ctx) : ctx_(std::move(ctx)) {}
ICP::~ICP() {
  if (scan_) mh_scan_destroy(scan_);
  for (auto& e : layer_scans_) mh_scan_destroy(e.second);
}

void ICP::setDeviceHook(double min_trans, double min_rot_rad, const CPose3D& checkpoint) {
  dev_hook_ = true;
  dev_hook_trans_ = min_trans;
  dev_hook_rot_ = min_rot_rad;
  dev_hook_chk_ = checkpoint;
}
void ICP::clearHooks() {
  dev_hook_ = false;
  iteration_hook_ = nullptr;
}

void ICP::attachToParameterSource(ParameterSource& s) {
  source_ = &s;
  for (auto& m : matchers_) m->attachToParameterSource(s);
  for (auto& v : solvers_) v->attachToParameterSource(s);
}

void ICP::initialize_matchers(const Config& seq) {
  matchers_.clear();
  for (size_t i = 0; i < seq.size(); i++) {
    auto m = create_matcher(seq.at(i)["class"].asString());
    m->initialize(seq.at(i)["params"]);
    m->attachToParameterSource(own_source_);
    matchers_.push_back(m);
  }
}
void ICP::initialize_solvers(const Config& seq) {
  solvers_.clear();
  for (size_t i = 0; i < seq.size(); i++) {
    auto s = create_solver(seq.at(i)["class"].asString());
    s->initialize(seq.at(i)["params"]);
    s->attachToParameterSource(own_source_);
    solvers_.push_back(s);
  }
}

// ICP::align updates "ICP_ITERATION" in the attached sources and re-realizes them every iteration [U]
void ICP::realize_iteration(uint32_t k) {
  std::map<std::string, double> vars = source_ ? source_->getVariableValues() : own_source_.getVariableValues();
  vars["ICP_ITERATION"] = (double)k;
  for (auto& m : matchers_) m->realizeWith(vars);
  for (auto& s : solvers_) s->realizeWith(vars);
}

// the two pipeline shapes the device loop implements: [Points_DistanceThreshold] (lidar3d-default.yaml:195-204) and
// [Point2Plane, Points_DistanceThreshold] on the same layers (lidar3d-ndt.yaml:195-210), with one Solver_GaussNewton
bool ICP::can_fuse() const {
  if (force_generic_ || (iteration_hook_ && !hook_replay_)) return false;
  if (matchers_.empty() || matchers_.size() > 2 || solvers_.size() != 1) return false;
  auto m = std::dynamic_pointer_cast<Matcher_Points_DistanceThreshold>(matchers_.back());
  auto s = std::dynamic_pointer_cast<Solver_GaussNewton>(solvers_[0]);
  if (!m || !s) return false;
  if (!(m->enabled && m->runFromIteration == 0 && m->runUpToIteration == 0 && m->pairingsPerPoint == 1 &&
        m->pointLayerMatches.size() == 1))  // (its weight: any -- the fused loop's solver takes it, round 5)
    return false;
  // U13: the single-pair chains and the one-launch loops pair a map point as often as it is nearest (can_fuse_layers takes it)
  if (!m->allowMatchAlreadyMatchedGlobalPoints) return false;
  if (matchers_.size() == 2) {
    auto pl = std::dynamic_pointer_cast<Matcher_Point2Plane>(matchers_[0]);
    if (!pl || !pl->enabled || pl->runFromIteration || pl->runUpToIteration || pl->pointLayerMatches.size() != 1) return false;
    const auto &a = pl->pointLayerMatches[0], &b = m->pointLayerMatches[0];
    if (a.global != b.global || a.local != b.local) return false;
  }
  return true;
}

// several point-layer pairs in one solve (lidar3d-dual-map.yaml:115-132, lidar3d-edges.yaml:120-129): one Solver_GaussNewton, only
// enabled Matcher_Points_DistanceThreshold with pairingsPerPoint 1, 2 to MH_MAX_LAYER_PAIRS entries in all -- or 1 to
// MH_MAX_LAYER_PAIRS when a matcher has allowMatchAlreadyMatchedGlobalPoints: false (U13: mh_icp_align_layers_opts is the one
// device loop that implements it, the default pipeline's single pair included) or an iteration gate.  Gated matchers
// (runFromIteration / runUpToIteration, lidar3d-near-far.yaml:183) only with fuseGatedMatchers / MOLA_HIP_FUSE_GATES=1
// (mh_icp_align_layers_gated); otherwise they keep the generic loop.  The same for pairingsPerPoint 2 .. MH_MAX_PAIRINGS_PER_POINT
// with fuseMultiPairings / MOLA_HIP_FUSE_KBEST=1 (mh_icp_align_layers_kbest), a single pair included.  A local layer named by two entries is paired again for each: only under
// MOLA_HIP_MATCHED_POINTS=again (skip would leave the second entry's points out, which mh_icp_align_layers does not do).
// Enabled Matcher_Point2Plane entries (KNN + PCA on point layers, rgbd.yaml:143-151) only with fusePlaneMatchers /
// MOLA_HIP_FUSE_PLANES=1 (mh_icp_align_layers_planes), gated ones under the gates switch as well; a single such pair included.
namespace {
// what the multi-layer loop reads of a matcher, whichever of its two kinds it is
struct FusedMatcher {
  const Matcher_Points_DistanceThreshold* pt = nullptr;
  const Matcher_Point2Plane* pl = nullptr;
  const Matcher* base() const { return pt ? static_cast<const Matcher*>(pt) : pl; }
  const std::vector<Matcher_Points_DistanceThreshold::LayerMatch>& entries() const { return pt ? pt->pointLayerMatches : pl->pointLayerMatches; }
  double threshold() const { return pt ? pt->threshold : pl->distanceThreshold; }
};
FusedMatcher fused_matcher(const Matcher::Ptr& mm) {
  FusedMatcher f;
  f.pt = dynamic_cast<const Matcher_Points_DistanceThreshold*>(mm.get());
  if (!f.pt) f.pl = dynamic_cast<const Matcher_Point2Plane*>(mm.get());
  return f;
}
}  // namespace

bool ICP::can_fuse_layers() const {
  if (force_generic_ || iteration_hook_) return false;
  if (matchers_.empty() || solvers_.size() != 1 || !std::dynamic_pointer_cast<Solver_GaussNewton>(solvers_[0])) return false;
  std::vector<std::string> locals;
  bool single_pair_ok = false;  // a unique or gated matcher: shapes only the multi-layer loop takes, a single pair included
  const bool gates_ok = molahip_host::fuse_allowed(molahip_host::plugin_switches().fuse_gates, fuse_gated_);
  const bool kbest_ok = molahip_host::fuse_allowed(molahip_host::plugin_switches().fuse_kbest, fuse_kbest_);
  const bool planes_ok = molahip_host::fuse_allowed(molahip_host::plugin_switches().fuse_planes, fuse_planes_);
  for (const auto& mm : matchers_) {
    if (auto pl = std::dynamic_pointer_cast<Matcher_Point2Plane>(mm)) {
      if (!planes_ok || !pl->enabled || pl->knn < 3 || pl->knn > MH_MAX_PLANE_KNN) return false;
      if ((pl->runFromIteration || pl->runUpToIteration) && !gates_ok) return false;
      single_pair_ok = single_pair_ok || !pl->pointLayerMatches.empty();
      for (const auto& lm : pl->pointLayerMatches) locals.push_back(lm.local);
      continue;
    }
    auto m = std::dynamic_pointer_cast<Matcher_Points_DistanceThreshold>(mm);
    if (!m || !m->enabled) return false;
    const bool multi = m->pairingsPerPoint != 1;  // (realizeWith has refused what is outside 1 .. MH_MAX_PAIRINGS_PER_POINT)
    if (multi && !(kbest_ok && m->pairingsPerPoint >= 1 && m->pairingsPerPoint <= MH_MAX_PAIRINGS_PER_POINT)) return false;
    const bool gated = m->runFromIteration || m->runUpToIteration;
    if (gated && !gates_ok) return false;
    single_pair_ok = single_pair_ok || ((!m->allowMatchAlreadyMatchedGlobalPoints || gated || multi) && !m->pointLayerMatches.empty());
    for (const auto& lm : m->pointLayerMatches) locals.push_back(lm.local);
  }
  if (locals.size() < (single_pair_ok ? 1u : 2u) || locals.size() > MH_MAX_LAYER_PAIRS) return false;
  std::sort(locals.begin(), locals.end());
  const bool shared = std::adjacent_find(locals.begin(), locals.end()) != locals.end();
  return !(shared && molahip_host::plugin_switches().matched_points == MH_MATCHED_POINTS_SKIP);
}

std::string ICP::alignPath() const {
  if (can_fuse()) return "single";
  if (can_fuse_layers()) return "layers";
  return "generic";
}

// the layers align_fused_layers needs: every global one a HashedVoxelPointCloud on the first one's context, every local one a
// PointCloud or a DevicePointCloud.  A plane matcher's global layer must carry no NDT statistics: on such a layer the generic
// route runs mh_nn_search_pt2pl (the per-voxel planes), which is another matcher than the loop's KNN + PCA.
static bool layer_inputs_ok(const std::vector<Matcher::Ptr>& matchers, const metric_map_t& pcLocal, const metric_map_t& pcGlobal) {
  const DeviceContext* ctx = nullptr;
  for (const auto& mm : matchers)
    for (const auto& lm : fused_matcher(mm).entries()) {
      auto g = pcGlobal.layers.find(lm.global);
      auto l = pcLocal.layers.find(lm.local);
      if (g == pcGlobal.layers.end() || l == pcLocal.layers.end()) return false;
      auto hv = std::dynamic_pointer_cast<HashedVoxelPointCloud>(g->second);
      if (!hv || (ctx && hv->context().get() != ctx)) return false;
      if (fused_matcher(mm).pl && std::dynamic_pointer_cast<NDT>(g->second)) return false;
      ctx = hv->context().get();
      // mh_icp_align_layers refuses a map of 2^30 or more records (records = points + two per voxel at most)
      mh_map_info info{};
      if (mh_map_get_info(hv->handle(), &info) != MH_OK || info.n_points + 2 * info.n_voxels >= (1ull << 30)) return false;
      if (!std::dynamic_pointer_cast<PointCloud>(l->second) && !std::dynamic_pointer_cast<DevicePointCloud>(l->second)) return false;
    }
  // ... and maps and scans on more than one context: a device local layer has to live on the maps' one
  for (const auto& mm : matchers)
    for (const auto& lm : fused_matcher(mm).entries()) {
      auto dev = std::dynamic_pointer_cast<DevicePointCloud>(pcLocal.layers.find(lm.local)->second);
      if (dev && dev->context().get() != ctx) return false;
    }
  return ctx != nullptr;
}

// ---------------------------------------------------------------- AlignBatcher
AlignBatcher::AlignBatcher(size_t participants) : active_(participants) {
  if (const char* e = getenv("MOLA_HIP_BATCH_SPLIT")) split_ = (size_t)std::max(1, atoi(e));
  solo_ = getenv("MOLA_HIP_BATCH_SOLO") != nullptr;  // every alignment on its own, as soon as it is asked for (A/B against the lock-step batches)
  no_solo_ = getenv("MOLA_HIP_BATCH_NO_SOLO") != nullptr;
}

// how many waiting requests make a batch: all active participants (split 1), or a share of them -- then two or more
// batches are in flight at once, each led by the thread that completed it, and nobody waits for the slowest alignment of
// ALL sequences (iteration counts differ by 5x from scan to scan), only for the slowest of its own batch
size_t AlignBatcher::threshold_locked() const {
  if (active_ < 4 || split_ <= 1) return active_;
  return std::max<size_t>(2, (active_ + split_ - 1) / split_);
}

// Everything that leaves waiting_ leaves it here, and leaves without its `lead` flag: a request whose flag is still set when its
// thread wakes is therefore still waiting (leave() used to swap the vector bare, a woken leader could then find it
// empty -- or holding NEWER requests -- and run a batch that did not contain itself).
void AlignBatcher::take_waiting_locked(std::vector<Request*>& batch) {
  batch.clear();
  batch.swap(waiting_);
  for (Request* r : batch) r->lead = false;
  in_flight_ += batch.size();
}

// a batch is due when enough requests wait -- or when everybody who is not waiting is inside a running batch already (then
// waiting longer only idles the device)
bool AlignBatcher::batch_due_locked() const {
  return !waiting_.empty() && (waiting_.size() >= threshold_locked() || waiting_.size() + in_flight_ >= active_);
}

void AlignBatcher::run_batch(std::vector<Request*>& batch) {
  if (batch.empty()) return;
  // the device work of this batch is issued by this thread alone; the mutex is NOT held (other participants queue up and
  // may start the next batch on their own contexts meanwhile: the C ABI is re-entrant across contexts)
  const size_t n = batch.size();
  const auto t_start = std::chrono::steady_clock::now();
  std::vector<mh_icp_result> results(n);
  std::vector<mh_status> sts(n, MH_OK);
  std::vector<std::string> errs(n);
  // the single-pair requests as one mh_icp_align_batch, the multi-layer ones as one mh_icp_align_layers_batch_planes
  for (const bool layers : {false, true}) {
    std::vector<size_t> idx;
    for (size_t i = 0; i < n; i++)
      if ((batch[i]->job.pairs != nullptr) == layers) idx.push_back(i);
    const size_t m = idx.size();
    if (!m) continue;
    std::vector<const mh_map*> maps(m);
    std::vector<const mh_scan*> scans(m);
    std::vector<mh_layer_job_planes> jobs(m);
    std::vector<mh_icp_params> params(m);
    std::vector<double> T(12 * m);
    std::vector<const mh_prior*> priors(m);
    std::vector<mh_icp_result> res(m);
    bool any_prior = false;
    for (size_t k = 0; k < m; k++) {
      const Request& rq = *batch[idx[k]];
      maps[k] = rq.map;
      scans[k] = rq.scan;
      jobs[k] = rq.job;
      params[k] = *rq.params;
      memcpy(&T[12 * k], rq.T, 12 * sizeof(double));
      priors[k] = rq.prior;
      any_prior = any_prior || rq.prior;
    }
    auto one = [&](size_t k) {
      return layers ? mh_icp_align_layers_planes(jobs[k].n_pairs, jobs[k].pairs, jobs[k].opts, jobs[k].gates, jobs[k].knn, jobs[k].planes,
                                                 &params[k], &T[12 * k], priors[k], &res[k], nullptr, nullptr, nullptr, nullptr, MH_MEM_HOST)
                    : mh_icp_align(maps[k], scans[k], &params[k], &T[12 * k], priors[k], &res[k], nullptr, nullptr, MH_MEM_HOST);
    };
    mh_status st = MH_OK;
    if (m == 1) {
      st = one(0);
    } else if (layers) {
      st = mh_icp_align_layers_batch_planes(m, jobs.data(), params.data(), 1, T.data(), any_prior ? priors.data() : nullptr, res.data(),
                                            nullptr);
    } else {
      st = mh_icp_align_batch(m, maps.data(), scans.data(), params.data(), 1, T.data(), any_prior ? priors.data() : nullptr,
                              res.data(), nullptr, MH_MEM_HOST);
    }
    const std::string err = st != MH_OK ? mh_last_error_string() : "";  // (thread-local in the library: read it on the thread that made the call)
    for (size_t k = 0; k < m; k++) {
      sts[idx[k]] = st;
      errs[idx[k]] = err;
    }
    if (st != MH_OK && m > 1) {
      // one job's bad argument or allocation failure must not fail the other sequences: once more, one by one, so that
      // every request gets its own status
      for (size_t k = 0; k < m; k++) {
        sts[idx[k]] = one(k);
        errs[idx[k]] = sts[idx[k]] != MH_OK ? mh_last_error_string() : "";
      }
    }
    for (size_t k = 0; k < m; k++) results[idx[k]] = res[k];
  }
  std::lock_guard<std::mutex> lk(mtx_);
  n_batches_++;
  n_jobs_ += n;
  t_run_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  t_assemble_ += std::chrono::duration<double>(t_start - batch[0]->arrived).count();
  in_flight_ -= n;
  if (batch_due_locked()) waiting_.front()->lead = true;  // (e.g. a participant left while this batch ran; woken by the notify below)
  for (size_t i = 0; i < n; i++) {
    *batch[i]->result = results[i];
    batch[i]->status = sts[i];
    batch[i]->error = errs[i];
    batch[i]->done = true;
  }
  cv_.notify_all();
}

mh_status AlignBatcher::alignLayers(const void* owner, const mh_layer_job_planes& job, const mh_icp_params* params,
                                    const double T_guess[12], const mh_prior* prior, mh_icp_result* result, std::string* error) {
  Request rq;
  rq.job = job; rq.params = params; rq.T = T_guess; rq.prior = prior; rq.result = result;
  // (no one-launch loops on the multi-layer path: nothing to ask the library; MOLA_HIP_BATCH_SOLO alone issues it at once)
  return submit(owner ? owner : (const void*)job.pairs, rq, solo_ ? 1 : 0, error);
}

void AlignBatcher::runOutside(const void* owner, const std::function<void()>& fn) {
  std::unique_lock<std::mutex> lk(mtx_);
  owners_[owner].aligns++;
  in_flight_ += 1;
  auto wake_leader = [&] {  // whoever waits for a batch waits for those who are not in flight: if that is nobody now, one of them leads it
    if (batch_due_locked()) {
      waiting_.front()->lead = true;
      cv_.notify_all();
    }
  };
  wake_leader();
  lk.unlock();
  try {
    fn();
  } catch (...) {
    lk.lock();
    in_flight_ -= 1;
    wake_leader();
    throw;
  }
  lk.lock();
  in_flight_ -= 1;
  wake_leader();
}

mh_status AlignBatcher::align(const void* owner, const mh_map* map, const mh_scan* scan, const mh_icp_params* params,
                              const double T_guess[12], const mh_prior* prior, mh_icp_result* result, std::string* error) {
  Request rq;
  rq.map = map; rq.scan = scan; rq.params = params; rq.T = T_guess; rq.prior = prior; rq.result = result;
  // An alignment the library runs as ONE launch (the default pipeline's ICP layers: <= 2048 points) gains nothing from a
  // lock-step batch and loses the wait for the others: it is issued on its own at once, as long as the loops of all active
  // participants fit the device together (4 sequences: 4450 against 3620 scans/s; with 8, whose loops would take turns, the
  // batches win: 4950 against 4100).
  int32_t solo = solo_ ? 1 : 0;
  if (!solo && !no_solo_) {
    size_t callers;
    {
      std::lock_guard<std::mutex> g(mtx_);
      callers = active_;
    }
    if (mh_icp_align_prefers_solo(scan, params, (uint32_t)callers, &solo) != MH_OK) solo = 0;
  }
  return submit(owner ? owner : (const void*)scan, rq, solo, error);
}

mh_status AlignBatcher::submit(const void* owner, Request& rq, int32_t solo, std::string* error) {
  std::unique_lock<std::mutex> lk(mtx_);
  rq.arrived = std::chrono::steady_clock::now();
  {
    OwnerState& os = owners_[owner];
    os.aligns++;  // this participant is past the filter set of its previous alignment count
    // A participant whose alignments run on their own is not in step with anybody: its prefetch worker's filter chain runs at
    // once instead of waiting for a set that only lock-step rounds complete (16 free-running sequences: 1.6 ms of every scan
    // were spent in `prefetch_wait`, 208 sets forced by the 2 ms net).
    static const bool filter_sets_always = getenv("MOLA_HIP_FILTER_SETS_ALWAYS") != nullptr;  // (A/B: the rendezvous also for solo callers)
    os.free_running = solo != 0 && !filter_sets_always;
    if (solo) last_solo_ = rq.arrived;
  }
  if (!pp_waiting_.empty()) cv_.notify_all();           // (a waiting filter worker may find its set complete now)
  if (solo) {
    in_flight_ += 1;
    // whoever waits for a batch waits for those who are not in flight: if that is nobody now, one of them leads it
    if (batch_due_locked()) {
      waiting_.front()->lead = true;
      cv_.notify_all();
    }
    std::vector<Request*> one{&rq};
    lk.unlock();
    run_batch(one);
    lk.lock();
    if (error) *error = rq.error;
    return rq.status;
  }
  waiting_.push_back(&rq);
  if (batch_due_locked()) {
    std::vector<Request*> batch;
    take_waiting_locked(batch);
    lk.unlock();
    run_batch(batch);
    lk.lock();
  } else {
    // Bounded: with three or more participants whose other alignments all run solo and never overlap, nobody's arrival makes
    // this request's batch due -- after the limit it leads whatever waits (a smaller batch: same results).
    static const auto limit_lockstep = std::chrono::microseconds([] {
      const char* e = getenv("MOLA_HIP_BATCH_WAIT_US");
      return e ? std::max(100, atoi(e)) : 3000;
    }());
    while (!rq.done) {
      // (while others' alignments run on their own -- one seen within the last few milliseconds -- nobody is coming to complete
      //  a round: this request leads what waits after a fraction of an alignment's duration)
      const bool free_run = (rq.arrived - last_solo_) < std::chrono::milliseconds(5);
      const auto limit = free_run ? std::chrono::microseconds(100) : limit_lockstep;
      const bool woke = cv_.wait_for(lk, limit, [&] { return rq.done || rq.lead; });
      if (rq.done) break;
      // `lead` set (or the limit reached) AND still among those waiting: whoever takes a batch clears the flags of its requests,
      // so a set flag means nobody has taken this one
      const bool still_waiting = std::find(waiting_.begin(), waiting_.end(), &rq) != waiting_.end();
      if (!still_waiting) continue;  // (taken by another leader meanwhile: its batch will set `done`)
      if (!woke) n_wait_timeouts_++;
      std::vector<Request*> batch;
      take_waiting_locked(batch);
      lk.unlock();
      run_batch(batch);
      lk.lock();
    }
  }
  if (error) *error = rq.error;
  return rq.status;
}

void AlignBatcher::run_filter_batch(std::vector<FilterRequest*>& batch) {
  const size_t n = batch.size();
  std::vector<const mh_scan*> raws(n);
  std::vector<mh_preprocess_params> params(n);
  std::vector<mh_scan*> maps(n), icps(n);
  for (size_t i = 0; i < n; i++) {
    raws[i] = batch[i]->raw;
    params[i] = *batch[i]->params;
    maps[i] = batch[i]->out_map;
    icps[i] = batch[i]->out_icp;
  }
  mh_status st = n == 1 ? mh_scan_preprocess(raws[0], &params[0], maps[0], icps[0])
                        : mh_scan_preprocess_batch(n, raws.data(), params.data(), sizeof(mh_preprocess_params), maps.data(), icps.data());
  std::vector<mh_status> sts(n, st);
  std::vector<std::string> errs(n, st != MH_OK ? mh_last_error_string() : "");
  if (st != MH_OK && n > 1)  // whose scan it was: one by one
    for (size_t i = 0; i < n; i++) {
      sts[i] = mh_scan_preprocess(raws[i], &params[i], maps[i], icps[i]);
      errs[i] = sts[i] != MH_OK ? mh_last_error_string() : "";
    }
  std::lock_guard<std::mutex> lk(mtx_);
  n_pp_batches_++;
  n_pp_jobs_ += n;
  for (size_t i = 0; i < n; i++) {
    batch[i]->status = sts[i];
    batch[i]->error = errs[i];
    batch[i]->done = true;
  }
  cv_.notify_all();
}

// complete = every active participant is past the set and every announced request of it (and of earlier sets) is here
bool AlignBatcher::filter_set_ready_locked(size_t set) const {
  if (set < pp_set_) return true;  // (its set went without it: a request that arrives late runs at once)
  for (const auto& kv : pp_pending_)
    if (kv.first <= set && kv.second > 0) return false;
  size_t past = 0;
  for (const auto& kv : owners_)
    past += (kv.second.free_running || kv.second.aligns > set || (kv.second.announced && kv.second.announced_set >= set)) ? 1 : 0;
  return past >= active_;
}

void AlignBatcher::take_filter_sets_upto(std::unique_lock<std::mutex>& lk, size_t set) {
  std::vector<FilterRequest*> batch, rest;
  for (auto* r : pp_waiting_) (r->set <= set ? batch : rest).push_back(r);
  pp_waiting_.swap(rest);
  if (set + 1 > pp_set_) pp_set_ = set + 1;
  for (auto* r : batch) r->taken = true;
  if (batch.empty()) return;
  lk.unlock();
  run_filter_batch(batch);
  lk.lock();
}

size_t AlignBatcher::announceFilter(const void* owner) {
  std::lock_guard<std::mutex> lk(mtx_);
  OwnerState& o = owners_[owner];
  if (o.free_running) return kNoFilterSet;  // (runs alone, at once: nobody waits for it, it waits for nobody)
  o.announced = true;
  o.announced_set = o.aligns;
  pp_pending_[o.aligns]++;
  return o.aligns;
}

void AlignBatcher::cancelAnnouncedFilter(const void* owner, size_t set) {
  (void)owner;
  if (set == kNoFilterSet) return;
  std::lock_guard<std::mutex> lk(mtx_);
  auto it = pp_pending_.find(set);
  if (it != pp_pending_.end() && it->second > 0 && --it->second == 0) pp_pending_.erase(it);
  cv_.notify_all();
}

mh_status AlignBatcher::preprocess(const void* owner, size_t set, const mh_scan* raw, const mh_preprocess_params* params,
                                   mh_scan* out_map, mh_scan* out_icp, std::string* error) {
  (void)owner;
  if (set == kNoFilterSet) {  // a free-running participant's request: its own launches, now
    const mh_status st = mh_scan_preprocess(raw, params, out_map, out_icp);
    if (st != MH_OK && error) *error = mh_last_error_string();
    std::lock_guard<std::mutex> lk(mtx_);
    n_pp_batches_++;
    n_pp_jobs_++;
    return st;
  }
  FilterRequest rq;
  rq.raw = raw; rq.params = params; rq.out_map = out_map; rq.out_icp = out_icp; rq.set = set;
  std::unique_lock<std::mutex> lk(mtx_);
  {
    auto it = pp_pending_.find(set);  // announced -> arrived
    if (it != pp_pending_.end() && it->second > 0 && --it->second == 0) pp_pending_.erase(it);
  }
  pp_waiting_.push_back(&rq);
  cv_.notify_all();  // (the arrival may be what another worker's set was waiting for)
  static const auto limit = std::chrono::microseconds([] {
    const char* e = getenv("MOLA_HIP_FILTER_SET_WAIT_US");
    return e ? std::max(0, atoi(e)) : 2000;
  }());
  while (!rq.done) {
    if (!rq.taken && filter_set_ready_locked(rq.set)) {
      take_filter_sets_upto(lk, rq.set);
      continue;
    }
    const bool woke = cv_.wait_for(lk, limit, [&] { return rq.done || (!rq.taken && filter_set_ready_locked(rq.set)); });
    if (woke || rq.taken) continue;
    n_pp_timeouts_++;  // nobody completed the set in time: everything up to this request's set runs now
    take_filter_sets_upto(lk, rq.set);
  }
  if (error) *error = rq.error;
  return rq.status;
}

void AlignBatcher::forgetOwner(const void* owner) {
  std::lock_guard<std::mutex> lk(mtx_);
  owners_.erase(owner);
  cv_.notify_all();
}

void AlignBatcher::leave() {
  std::unique_lock<std::mutex> lk(mtx_);
  if (active_ > 0) active_--;
  cv_.notify_all();  // (fewer participants: a waiting filter set may be complete now)
  if (batch_due_locked()) {
    // the others were only waiting for this one
    std::vector<Request*> batch;
    take_waiting_locked(batch);
    lk.unlock();
    run_batch(batch);
  }
}

void ICP::align(const metric_map_t& pcLocal, const metric_map_t& pcGlobal, const TPose3D& guess, const Parameters& p,
                Results& result, const std::optional<CPose3DPDFGaussianInf>& prior) {
  result = Results();
  const CPose3D g(guess);
  if (can_fuse()) {
    auto m = std::static_pointer_cast<Matcher_Points_DistanceThreshold>(matchers_.back());
    last_fused_ = true;
    const std::string& lname = m->pointLayerMatches[0].local;
    auto it = pcLocal.layers.find(lname);
    auto dev = it != pcLocal.layers.end() ? std::dynamic_pointer_cast<DevicePointCloud>(it->second) : nullptr;
    align_fused(dev ? nullptr : &local_layer(pcLocal, lname), dev.get(), global_layer(pcGlobal, m->pointLayerMatches[0].global),
                g, p, result, prior);
  } else if (can_fuse_layers() && layer_inputs_ok(matchers_, pcLocal, pcGlobal)) {
    last_fused_ = true;
    align_fused_layers(pcLocal, pcGlobal, g, p, result, prior);
  } else {
    last_fused_ = false;
    // (no batched form: beside a batcher the participant counts as busy meanwhile, so nobody waits for a request it will not make)
    if (batcher_) batcher_->runOutside(batch_owner_, [&] { align_generic(pcLocal, pcGlobal, g, p, result, prior); });
    else align_generic(pcLocal, pcGlobal, g, p, result, prior);
  }
}

// the per-align trace file of Parameters::generateDebugFiles (see the header)
static void write_debug_file(const Parameters& p, const CPose3D& guess, const mh_icp_result& r, const std::vector<mh_icp_iter>& trace,
                             size_t n_local) {
  static std::atomic<uint64_t> counter{0};
  std::string path = p.debugFileNameFormat;
  const std::string id = std::to_string(counter++);
  for (size_t pos; (pos = path.find("$UNIQUE_ID")) != std::string::npos;) path.replace(pos, 10, id);
  for (const char* var : {"$LOCAL_ID", "$LOCAL_LABEL", "$GLOBAL_ID", "$GLOBAL_LABEL"})
    for (size_t pos; (pos = path.find(var)) != std::string::npos;) path.erase(pos, strlen(var));
  const size_t slash = path.find_last_of('/');
  if (slash != std::string::npos) {
    std::string dir;
    for (size_t i = 0; i <= slash; i++) {  // mkdir -p
      dir += path[i];
      if (path[i] == '/') (void)mkdir(dir.c_str(), 0755);
    }
  }
  FILE* f = fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("generateDebugFiles: cannot write " + path);
  auto pose = [&](const double* T) {
    fprintf(f, "[");
    for (int i = 0; i < 12; i++) fprintf(f, "%s%.17g", i ? ", " : "", T[i]);
    fprintf(f, "]");
  };
  fprintf(f, "{\n \"format\": \"molahip-icplog-json-1\", \"n_local_points\": %zu, \"max_iterations\": %u,\n \"initial_guess\": ", n_local, p.maxIterations);
  pose(guess.T);
  fprintf(f, ",\n \"iterations\": [\n");
  const uint32_t cnt = std::min<uint32_t>(p.maxIterations, r.n_iterations + 1);
  for (uint32_t k = 0; k < cnt; k++) {
    fprintf(f, "  {\"iteration\": %u, \"n_pairs\": %u, \"threshold\": %.17g, \"kernel_param\": %.17g, \"delta_trans\": %.17g, \"delta_rot\": %.17g, \"pose\": ",
            k, trace[k].n_pairs, trace[k].threshold, trace[k].kernel_param, trace[k].delta_trans, trace[k].delta_rot);
    pose(trace[k].T);
    fprintf(f, "}%s\n", k + 1 < cnt ? "," : "");
  }
  fprintf(f, " ],\n \"n_iterations\": %u, \"termination\": \"%s\", \"quality\": %.17g, \"n_final_pairs\": %u,\n \"final_pose\": ",
          r.n_iterations, enum2str((IterTermReason)r.termination_reason), r.quality, r.n_final_pairs);
  pose(r.T);
  fprintf(f, "\n}\n");
  fclose(f);
}

// The thresholds are functions of ICP_ITERATION only once the caller's variables are fixed (LidarOdometry.cpp:1571-1635
// publishes them before align): all iterations evaluated up front.  The result is kept with the VALUES of the variables
// the formulas read, so that a caller who knows them early (the odometry driver, while the device is busy with the
// key-frame update of the previous scan) can have the work done before align() needs it: 300 iterations x 2-3 formulas
// were 40 us of a 1 ms scan with the device idle.
void ICP::prepare_schedule(uint32_t n_iterations) {
  auto m = std::static_pointer_cast<Matcher_Points_DistanceThreshold>(matchers_.back());
  auto s = std::static_pointer_cast<Solver_GaussNewton>(solvers_[0]);
  auto mpl = matchers_.size() == 2 ? std::static_pointer_cast<Matcher_Point2Plane>(matchers_[0]) : nullptr;
  // formulas compiled once and bound to one copy of the variables; only ICP_ITERATION is swept (in place)
  std::map<std::string, double> vars = source_ ? source_->getVariableValues() : own_source_.getVariableValues();
  double& it_var = vars["ICP_ITERATION"];
  it_var = 0.0;
  const auto bm = m->bind(vars);
  const auto bs = s->bind(vars);
  Parameterizable::Binding bp;
  if (mpl) bp = mpl->bind(vars);
  std::vector<double> key;
  for (const Parameterizable::Binding* b : {&bm, &bs, (const Parameterizable::Binding*)&bp})
    for (const auto& item : b->items)
      for (const double* v : item.second) key.push_back(*v);
  if (sched_.valid && sched_.key == key && sched_.thr.size() >= n_iterations) return;
  sched_.valid = false;
  sched_.key = key;
  sched_.thr.assign(n_iterations, 0.0);
  sched_.kp.assign(n_iterations, 0.0);
  sched_.plthr.assign(n_iterations, 0.0);
  for (uint32_t k = 0; k < n_iterations; k++) {
    it_var = (double)k;
    bm.realize();
    bs.realize();
    bp.realize();
    sched_.thr[k] = m->threshold;
    sched_.kp[k] = s->robustKernelParam;
    if (mpl) sched_.plthr[k] = mpl->distanceThreshold;
  }
  sched_.valid = true;
}

void ICP::precomputeSchedule(uint32_t n_iterations) {
  if (!n_iterations) return;
  if (can_fuse())
    prepare_schedule(n_iterations);
  else if (can_fuse_layers())
    prepare_layer_schedule(n_iterations);
  else
    return;
  realize_iteration(0);  // (the members the formulas write are left as align() leaves them)
}

// prepare_schedule for the multi-layer shapes: every matcher's threshold and the solver's kernel parameter, formulas bound once,
// one realize per iteration; kept with the values of the variables the formulas read
void ICP::prepare_layer_schedule(uint32_t n_iterations) {
  auto s = std::static_pointer_cast<Solver_GaussNewton>(solvers_[0]);
  std::vector<FusedMatcher> ms;  // (a plane matcher's schedule: its distanceThreshold)
  for (const auto& mm : matchers_) ms.push_back(fused_matcher(mm));
  std::map<std::string, double> vars = source_ ? source_->getVariableValues() : own_source_.getVariableValues();
  double& it_var = vars["ICP_ITERATION"];
  it_var = 0.0;
  std::vector<Parameterizable::Binding> bm;
  for (const auto& mm : matchers_) bm.push_back(mm->bind(vars));
  const auto bs = s->bind(vars);
  std::vector<double> key;
  for (const Parameterizable::Binding* b : {&bs})
    for (const auto& item : b->items)
      for (const double* v : item.second) key.push_back(*v);
  for (const auto& b : bm)
    for (const auto& item : b.items)
      for (const double* v : item.second) key.push_back(*v);
  key.push_back((double)ms.size());
  if (layer_sched_.valid && layer_sched_.key == key && layer_sched_.kp.size() >= n_iterations) return;
  layer_sched_.valid = false;
  layer_sched_.key = key;
  layer_sched_.thr.assign(ms.size(), std::vector<double>(n_iterations, 0.0));
  layer_sched_.kp.assign(n_iterations, 0.0);
  for (uint32_t k = 0; k < n_iterations; k++) {
    it_var = (double)k;
    for (const auto& b : bm) b.realize();
    bs.realize();
    for (size_t j = 0; j < ms.size(); j++) layer_sched_.thr[j][k] = ms[j].threshold();
    layer_sched_.kp[k] = s->robustKernelParam;
  }
  layer_sched_.valid = true;
}

void ICP::align_fused(const PointCloud* host_local, const DevicePointCloud* dev_local, const HashedVoxelPointCloud& global,
                      const CPose3D& guess, const Parameters& p, Results& result,
                      const std::optional<CPose3DPDFGaussianInf>& prior) {
  auto m = std::static_pointer_cast<Matcher_Points_DistanceThreshold>(matchers_.back());
  auto s = std::static_pointer_cast<Solver_GaussNewton>(solvers_[0]);
  auto mpl = matchers_.size() == 2 ? std::static_pointer_cast<Matcher_Point2Plane>(matchers_[0]) : nullptr;
  // the thresholds are functions of ICP_ITERATION only once the caller's variables are fixed for this call
  // (LidarOdometry.cpp:1571-1635 publishes them before align): evaluate them for every iteration up front
  const auto t_setup0 = std::chrono::steady_clock::now();
  prepare_schedule(p.maxIterations);  // (a no-op when precomputeSchedule() ran on the same values of the variables)
  const std::vector<double>&thr = sched_.thr, &kp = sched_.kp, &plthr = sched_.plthr;
  {  // the largest pair distance of the whole call, before the map's handle is read (an occupancy map sizes its search voxel by it)
    double radius = thr.empty() ? 0.0 : *std::max_element(thr.begin(), thr.end());
    if (mpl && !plthr.empty()) radius = std::max(radius, *std::max_element(plthr.begin(), plthr.end()));
    global.prepareSearch(radius);
  }
  if (p.maxIterations) realize_iteration(0);
  mh_icp_params ip{};
  ip.max_iterations = p.maxIterations;
  ip.min_abs_step_trans = p.minAbsStep_trans;
  ip.min_abs_step_rot = p.minAbsStep_rot;
  ip.threshold = thr.data();
  ip.kernel_param = kp.data();
  ip.threshold_angular_deg = m->thresholdAngularDeg;
  ip.pt2pl_threshold = mpl ? plthr.data() : nullptr;
  ip.gn = gn_params_of(*s);
  ip.gn.weight_pt2pt = m->pointLayerMatches[0].weight;  // pointLayerMatches {..., weight} (yaml:203-204)
  if (mpl) ip.gn.weight_pt2pl = mpl->pointLayerMatches[0].weight;
  ip.hook_enabled = dev_hook_ ? 1u : 0u;
  ip.hook_min_trans = dev_hook_trans_;
  ip.hook_min_rot = dev_hook_rot_;
  memcpy(ip.hook_checkpoint, dev_hook_chk_.T, sizeof(ip.hook_checkpoint));
  ip.compute_covariance = 1;
  ip.cov_findif_xyz = 1e-7;
  ip.cov_findif_ang = 1e-7;
  molahip_host::apply_switches(ip, molahip_host::plugin_switches());  // MOLA_HIP_* overrides, if any are set
  if (p.maxIterations > full_budget_) full_budget_ = p.maxIterations;
  const int call_kind = p.maxIterations < full_budget_ ? 1 : 0;
  ip.expected_iterations = last_iterations_[call_kind];
  mh_scan* scan = nullptr;
  PointCloud downloaded;  // only when a device layer's final pairings are requested
  if (dev_local) {
    scan = dev_local->handle();  // already resident: no upload
  } else {
    const PointCloud& hl = *host_local;
    if (scan_ && scan_ctx_ != global.context()) {  // the staging layer lives in the map's context: follow the map
      mh_scan_destroy(scan_);
      scan_ = nullptr;
    }
    if (!scan_) {
      scan_ctx_ = global.context();  // (kept alive: the layer must not outlive its context)
      check(mh_scan_create(scan_ctx_->get(), hl.x.data(), hl.y.data(), hl.z.data(), hl.size(), MH_MEM_HOST, &scan_),
            "mh_scan_create");
    } else
      check(mh_scan_update(scan_, hl.x.data(), hl.y.data(), hl.z.data(), hl.size(), MH_MEM_HOST), "mh_scan_update");
    scan = scan_;
  }
  mh_prior pr;
  if (prior) fill_prior(prior, pr);
  last_setup_seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_setup0).count();
  mh_icp_result r{};
  const size_t n = dev_local ? dev_local->size() : host_local->size();
  const bool want_pairs = keep_pairings_;
  std::vector<uint32_t> li(want_pairs ? n : 0), gi(li.size());
  std::vector<float> gx(li.size()), gy(li.size()), gz(li.size()), d2(li.size());
  mh_pairs_out po{li.data(), gi.data(), gx.data(), gy.data(), gz.data(), d2.data()};
  std::vector<mh_icp_iter> trace(p.generateDebugFiles ? p.maxIterations : 0);
  if (iteration_hook_) {
    // an opaque host hook on the fused loop: replay it on the traced poses (molahip_host/hook_replay.h)
    ip.hook_enabled = 0;
    auto run = [&](uint32_t budget, mh_icp_iter* tr) {
      mh_icp_params q = ip;
      q.max_iterations = budget;
      mh_icp_result rr{};
      check(mh_icp_align(global.handle(), scan, &q, guess.T, prior ? &pr : nullptr, &rr, tr, want_pairs ? &po : nullptr,
                         MH_MEM_HOST), "mh_icp_align");
      if (tr && !trace.empty()) std::copy(tr, tr + budget, trace.begin());
      return rr;
    };
    auto hook = [&](uint32_t k, const double* T) {
      OptimalTF_Result cur;
      memcpy(cur.optimalPose.T, T, sizeof(cur.optimalPose.T));
      IterationHook_Input in;
      in.currentIteration = k;
      in.currentSolution = &cur;
      return iteration_hook_(in).request_stop;
    };
    r = molahip_host::align_with_replayed_hook(p.maxIterations, run, hook);
  } else if (batcher_ && trace.empty() && !want_pairs) {
    // several sequences in one process: this alignment joins the others' (AlignBatcher)
    std::string err;
    const mh_status st = batcher_->align(batch_owner_, global.handle(), scan, &ip, guess.T, prior ? &pr : nullptr, &r, &err);
    if (st != MH_OK) throw std::runtime_error(std::string("mh_icp_align_batch: ") + mh_status_string(st) + ": " + err);
  } else {
    check(mh_icp_align(global.handle(), scan, &ip, guess.T, prior ? &pr : nullptr, &r, trace.empty() ? nullptr : trace.data(),
                       want_pairs ? &po : nullptr, MH_MEM_HOST), "mh_icp_align");
  }
  if (p.generateDebugFiles) write_debug_file(p, guess, r, trace, n);
  last_iterations_[call_kind] = r.n_iterations + (r.termination_reason == MH_TERM_MAX_ITERATIONS ? 0u : 1u);
  last_polls_ = r.n_host_polls;
  last_enqueued_ = r.n_enqueued_iterations;
  memcpy(result.optimal_tf.mean.T, r.T, sizeof(r.T));
  memcpy(result.optimal_tf.cov, r.cov, sizeof(r.cov));
  result.quality = r.quality;
  result.nIterations = r.n_iterations;
  result.terminationReason = (IterTermReason)r.termination_reason;
  Pairings& fp = result.finalPairings;
  fp.potential_pairings = r.potential_pairings;
  if (!want_pairs) return;
  if (dev_local) dev_local->download(downloaded.x, downloaded.y, downloaded.z);
  const PointCloud& local = dev_local ? downloaded : *host_local;
  if (r.n_final_pairs_pt2pl) {
    std::vector<uint32_t> qli(n);
    std::vector<float> a[6];
    for (auto& v : a) v.resize(n);
    mh_pairs_pl_out qo{qli.data(), a[0].data(), a[1].data(), a[2].data(), a[3].data(), a[4].data(), a[5].data()};
    uint64_t nq = 0;
    check(mh_icp_get_pt2pl_pairs(scan, &qo, MH_MEM_HOST, &nq), "mh_icp_get_pt2pl_pairs");
    append_pl_pairs(local, qli, a, nq, fp);
  }
  for (uint32_t k = 0; k < r.n_final_pairs - r.n_final_pairs_pt2pl; k++) {
    fp.localIdx.push_back(li[k]);
    fp.globalIdx.push_back(gi[k]);
    fp.lx.push_back(local.x[li[k]]);
    fp.ly.push_back(local.y[li[k]]);
    fp.lz.push_back(local.z[li[k]]);
    fp.gx.push_back(gx[k]);
    fp.gy.push_back(gy[k]);
    fp.gz.push_back(gz[k]);
    fp.errSq.push_back(d2[k]);
  }
}

// The multi-layer shapes on the device loop (mh_icp_align_layers).  Pairs in align_generic's matching order: matchers in list
// order, entries in pointLayerMatches order.  With a batcher set (and neither a trace nor the pairings wanted) the alignment joins
// those of the other sequences: AlignBatcher::alignLayers, mh_icp_align_layers_batch_planes with the job as described here
// (MOLA_HIP_BATCH_OPTS=0: an alignment with a unique pair, a gate or pairingsPerPoint > 1 runs on its own instead;
// MOLA_HIP_BATCH_PLANES=0: likewise one with a Matcher_Point2Plane pair).
void ICP::align_fused_layers(const metric_map_t& pcLocal, const metric_map_t& pcGlobal, const CPose3D& guess, const Parameters& p,
                             Results& result, const std::optional<CPose3DPDFGaussianInf>& prior) {
  const auto t_setup0 = std::chrono::steady_clock::now();
  auto s = std::static_pointer_cast<Solver_GaussNewton>(solvers_[0]);
  std::vector<FusedMatcher> ms;
  for (const auto& mm : matchers_) ms.push_back(fused_matcher(mm));
  // every matcher's threshold schedule and the solver's kernel parameter (a no-op when precomputeSchedule() ran on the same
  // values of the variables)
  const uint32_t mi = p.maxIterations;
  prepare_layer_schedule(mi ? mi : 1);
  const std::vector<std::vector<double>>& thr = layer_sched_.thr;
  const std::vector<double>& kp = layer_sched_.kp;
  if (mi) realize_iteration(0);
  mh_icp_params ip{};
  ip.max_iterations = mi;
  ip.min_abs_step_trans = p.minAbsStep_trans;
  ip.min_abs_step_rot = p.minAbsStep_rot;
  ip.threshold = thr[0].data();  // (not read: every pair carries its own)
  ip.kernel_param = kp.data();
  ip.gn = gn_params_of(*s);
  ip.hook_enabled = dev_hook_ ? 1u : 0u;
  ip.hook_min_trans = dev_hook_trans_;
  ip.hook_min_rot = dev_hook_rot_;
  memcpy(ip.hook_checkpoint, dev_hook_chk_.T, sizeof(ip.hook_checkpoint));
  ip.compute_covariance = 1;
  ip.cov_findif_xyz = 1e-7;
  ip.cov_findif_ang = 1e-7;
  molahip_host::apply_switches(ip, molahip_host::plugin_switches());
  if (mi > full_budget_) full_budget_ = mi;
  const int call_kind = mi < full_budget_ ? 1 : 0;
  ip.expected_iterations = last_iterations_[call_kind];
  // the pairs; host local layers are staged in the maps' context, once per layer name
  struct Entry {
    const PointCloud* host = nullptr;
    const DevicePointCloud* dev = nullptr;
  };
  molahip_host::LayerJobBuilder jb;  // each entry with its matcher's options
  std::vector<Entry> entries;
  const auto& ctx0 = global_layer(pcGlobal, ms[0].entries()[0].global).context();
  if (scan_ctx_ && scan_ctx_ != ctx0) {
    for (auto& e : layer_scans_) mh_scan_destroy(e.second);
    layer_scans_.clear();
    if (scan_) mh_scan_destroy(scan_);
    scan_ = nullptr;
  }
  scan_ctx_ = ctx0;
  // First every global layer is told the largest pair distance that ANY pair of this call can accept on it (an occupancy map
  // sizes its search voxel by it, and growing replaces its search map), only then are the handles read: a handle taken before a
  // later pair's larger radius would name a map that no longer exists.
  {
    std::map<std::string, double> radius_of;
    for (size_t j = 0; j < ms.size(); j++) {
      double radius = thr[j].empty() ? 0.0 : *std::max_element(thr[j].begin(), thr[j].end());
      if (ms[j].pl) radius = std::max(radius, ms[j].pl->searchRadius);
      for (const auto& lm : ms[j].entries()) radius_of[lm.global] = std::max(radius_of[lm.global], radius);
    }
    for (const auto& [name, radius] : radius_of) global_layer(pcGlobal, name).prepareSearch(radius);
  }
  std::map<std::string, bool> staged;
  for (size_t j = 0; j < ms.size(); j++)
    for (const auto& lm : ms[j].entries()) {
      Entry e;
      auto it = pcLocal.layers.find(lm.local);
      e.dev = std::dynamic_pointer_cast<DevicePointCloud>(it->second).get();
      mh_scan* scan = nullptr;
      if (e.dev) {
        scan = e.dev->handle();
      } else {
        e.host = &local_layer(pcLocal, lm.local);
        mh_scan*& st = layer_scans_[lm.local];
        if (!staged[lm.local]) {
          const PointCloud& hl = *e.host;
          if (!st)
            check(mh_scan_create(ctx0->get(), hl.x.data(), hl.y.data(), hl.z.data(), hl.size(), MH_MEM_HOST, &st), "mh_scan_create");
          else
            check(mh_scan_update(st, hl.x.data(), hl.y.data(), hl.z.data(), hl.size(), MH_MEM_HOST), "mh_scan_update");
          staged[lm.local] = true;
        }
        scan = st;
      }
      mh_layer_pair lp{};
      lp.map = global_layer(pcGlobal, lm.global).handle();
      lp.scan = scan;
      lp.threshold = thr[j].data();
      lp.threshold_angular_deg = ms[j].pt ? ms[j].pt->thresholdAngularDeg : 0.0;
      lp.weight = lm.weight;  // (a plane matcher's entries may differ in weight here: every pair scales its own rows)
      mh_layer_pair_plane lpl{};
      if (ms[j].pl) {
        lpl.knn = ms[j].pl->knn;
        lpl.minimum_plane_points = ms[j].pl->minimumPlanePoints;
        lpl.plane_eigen_threshold = ms[j].pl->planeEigenThreshold;
        lpl.search_radius = ms[j].pl->searchRadius;
      }
      // U13: allowMatchAlreadyMatchedGlobalPoints false (a plane pairing names no map point: nothing to claim, whatever the
      // matcher says); runFromIteration / runUpToIteration; pairingsPerPoint
      jb.push(lp, ms[j].pt && !ms[j].pt->allowMatchAlreadyMatchedGlobalPoints,
              mh_layer_pair_gates{ms[j].base()->runFromIteration, ms[j].base()->runUpToIteration},
              ms[j].pt ? (uint32_t)ms[j].pt->pairingsPerPoint : 1u, lpl);
      entries.push_back(e);
    }
  mh_prior pr;
  if (prior) fill_prior(prior, pr);
  last_setup_seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_setup0).count();
  const bool want_pairs = keep_pairings_;
  const mh_layer_job_planes job = jb.job();
  const size_t np = jb.size();
  std::vector<std::vector<uint32_t>> li(np), gi(np);
  std::vector<std::vector<float>> gx(np), gy(np), gz(np), d2(np);
  std::vector<mh_pairs_out> po(np);
  std::vector<mh_pairs_pl_out> ppl(np);  // a plane pair's final pairings: li | centroid in gx gy gz | normal in pn
  std::vector<std::array<std::vector<float>, 3>> pn(np);
  std::vector<uint64_t> counts(np, 0);
  for (size_t i = 0; want_pairs && i < np; i++) {
    const size_t n = (entries[i].dev ? entries[i].dev->size() : entries[i].host->size()) * (size_t)jb.pairings_per_point(i);
    li[i].resize(n); gx[i].resize(n); gy[i].resize(n); gz[i].resize(n);
    if (jb.is_plane(i)) {
      for (auto& v : pn[i]) v.resize(n);
      ppl[i] = mh_pairs_pl_out{li[i].data(), gx[i].data(), gy[i].data(), gz[i].data(), pn[i][0].data(), pn[i][1].data(), pn[i][2].data()};
      continue;
    }
    gi[i].resize(n); d2[i].resize(n);
    po[i] = mh_pairs_out{li[i].data(), gi[i].data(), gx[i].data(), gy[i].data(), gz[i].data(), d2[i].data()};
  }
  mh_icp_result r{};
  std::vector<mh_icp_iter> trace(p.generateDebugFiles ? mi : 0);
  auto solo = [&] {
    check(mh_icp_align_layers_planes(job.n_pairs, job.pairs, job.opts, job.gates, job.knn, job.planes, &ip, guess.T,
                                     prior ? &pr : nullptr, &r, trace.empty() ? nullptr : trace.data(),
                                     want_pairs ? po.data() : nullptr, (want_pairs && jb.has_plane()) ? ppl.data() : nullptr,
                                     counts.data(), MH_MEM_HOST), "mh_icp_align_layers_planes");
  };
  if (batcher_ && jb.has_plane() && (!molahip_host::plugin_switches().batch_planes || !trace.empty() || want_pairs)) {
    // (MOLA_HIP_BATCH_PLANES=0, the A/B against mh_icp_align_layers_batch_planes, or a trace / the pairings wanted: on its own
    // beside the batches, the participant counted as busy meanwhile)
    batcher_->runOutside(batch_owner_, solo);
  } else if (batcher_ && (jb.has_unique() || jb.has_gate() || jb.has_knn()) && !molahip_host::plugin_switches().batch_opts) {
    // (MOLA_HIP_BATCH_OPTS=0, the A/B against the batch: on its own, the participant counted as busy
    // meanwhile -- as align_generic)
    batcher_->runOutside(batch_owner_, solo);
  } else if (batcher_ && trace.empty() && !want_pairs) {
    std::string err;
    const mh_status st = batcher_->alignLayers(batch_owner_, job, &ip, guess.T, prior ? &pr : nullptr, &r, &err);
    if (st != MH_OK) throw std::runtime_error(std::string("mh_icp_align_layers_batch: ") + mh_status_string(st) + ": " + err);
  } else {
    solo();
  }
  if (p.generateDebugFiles) write_debug_file(p, guess, r, trace, (size_t)r.potential_pairings);
  last_iterations_[call_kind] = r.n_iterations + (r.termination_reason == MH_TERM_MAX_ITERATIONS ? 0u : 1u);
  last_polls_ = r.n_host_polls;
  last_enqueued_ = r.n_enqueued_iterations;
  memcpy(result.optimal_tf.mean.T, r.T, sizeof(r.T));
  memcpy(result.optimal_tf.cov, r.cov, sizeof(r.cov));
  result.quality = r.quality;
  result.nIterations = r.n_iterations;
  result.terminationReason = (IterTermReason)r.termination_reason;
  Pairings& fp = result.finalPairings;
  fp.potential_pairings = r.potential_pairings;
  if (!want_pairs) return;
  for (size_t i = 0; i < np; i++) {
    PointCloud downloaded;
    if (entries[i].dev && counts[i]) entries[i].dev->download(downloaded.x, downloaded.y, downloaded.z);
    const PointCloud& local = entries[i].dev ? downloaded : *entries[i].host;
    if (jb.is_plane(i)) {
      const std::vector<float> a[6] = {gx[i], gy[i], gz[i], pn[i][0], pn[i][1], pn[i][2]};
      append_pl_pairs(local, li[i], a, counts[i], fp);
      continue;
    }
    for (uint64_t k = 0; k < counts[i]; k++) {
      fp.localIdx.push_back(li[i][k]);
      fp.globalIdx.push_back(gi[i][k]);
      fp.lx.push_back(local.x[li[i][k]]);
      fp.ly.push_back(local.y[li[i][k]]);
      fp.lz.push_back(local.z[li[i][k]]);
      fp.gx.push_back(gx[i][k]);
      fp.gy.push_back(gy[i][k]);
      fp.gz.push_back(gz[i][k]);
      fp.errSq.push_back(d2[i][k]);
    }
  }
}

// matcher/solver-granular loop: the structure of mp2p_icp::ICP::align [U] with every numeric step on
// the device; used for custom pipelines and arbitrary host iteration hooks
void ICP::align_generic(const metric_map_t& pcLocal, const metric_map_t& pcGlobal, const CPose3D& guess, const Parameters& p,
                        Results& result, const std::optional<CPose3DPDFGaussianInf>& prior) {
  OptimalTF_Result cur;
  cur.optimalPose = guess;
  CPose3D prev = guess;
  Pairings pairings;
  for (result.nIterations = 0; result.nIterations < p.maxIterations; result.nIterations++) {
    const uint32_t k = (uint32_t)result.nIterations;
    realize_iteration(k);
    MatchContext mc;
    mc.icpIteration = k;
    pairings = Pairings();
    for (auto& m : matchers_) m->match(pcGlobal, pcLocal, cur.optimalPose, mc, pairings);
    if (pairings.empty()) {
      result.terminationReason = IterTermReason::NoPairings;
      break;
    }
    SolverContext sc;
    sc.guessRelativePose = cur.optimalPose;
    sc.prior = prior;
    sc.icpIteration = k;
    bool ok = false;
    for (auto& s : solvers_) {
      ok = s->optimal_pose(pairings, cur, sc);
      if (ok) break;
    }
    if (!ok) {
      result.terminationReason = IterTermReason::SolverError;
      break;
    }
    // stall test on log_SE3(prev^-1 (+) cur): |V^-1 t| and |w| (lidar3d-default.yaml:174-175)
    double xi_t, xi_r;
    se3_log_norms(cur.optimalPose - prev, xi_t, xi_r);
    if (xi_t < p.minAbsStep_trans && xi_r < p.minAbsStep_rot) {
      result.terminationReason = IterTermReason::Stalled;
      break;
    }
    if (iteration_hook_) {
      IterationHook_Input hi;
      hi.currentIteration = k;
      hi.currentSolution = &cur;
      if (iteration_hook_(hi).request_stop) {
        result.terminationReason = IterTermReason::HookRequest;
        break;
      }
    } else if (dev_hook_) {
      const CPose3D hd = cur.optimalPose - dev_hook_chk_;
      if (hd.translationNorm() > dev_hook_trans_ || hd.rotationAngle() > dev_hook_rot_) {
        result.terminationReason = IterTermReason::HookRequest;
        break;
      }
    }
    prev = cur.optimalPose;
  }
  if (result.nIterations >= p.maxIterations) result.terminationReason = IterTermReason::MaxIterations;
  result.quality = pairings.empty() ? 0.0 : quality_.evaluate(pairings);
  result.optimal_tf.mean = cur.optimalPose;
  mh_pairs_pt2pt pp{pairings.lx.data(), pairings.ly.data(), pairings.lz.data(), pairings.gx.data(), pairings.gy.data(),
                    pairings.gz.data(), pairings.localIdx.size()};
  mh_pairs_pt2pl pl{pairings.pl_lx.data(), pairings.pl_ly.data(), pairings.pl_lz.data(), pairings.pl_cx.data(),
                    pairings.pl_cy.data(), pairings.pl_cz.data(), pairings.pl_nx.data(), pairings.pl_ny.data(),
                    pairings.pl_nz.data(), pairings.pl_lx.size()};
  if (!ctx_) ctx_ = DeviceContext::Default();
  check(mh_covariance(ctx_->get(), &pp, &pl, MH_MEM_HOST, cur.optimalPose.T, 1e-7, 1e-7, result.optimal_tf.cov), "mh_covariance");
  result.finalPairings = std::move(pairings);
}

std::tuple<ICP::Ptr, Parameters> icp_pipeline_from_yaml(const Config& c, std::shared_ptr<DeviceContext> ctx) {
  const std::string cn = c.getOr("class_name", "mp2p_icp::ICP");
  if (cn != "mp2p_icp::ICP" && cn != "mp2p_icp_hip::ICP") throw std::runtime_error("ICP class '" + cn + "' is not available");
  auto icp = std::make_shared<ICP>(std::move(ctx));
  Parameters p;
  if (c.has("params")) p.load_from(c["params"]);
  icp->initialize_solvers(c["solvers"]);
  icp->initialize_matchers(c["matchers"]);
  if (c.has("quality")) {
    const Config& q = c["quality"];
    for (size_t i = 0; i < q.size(); i++) {
      const std::string qc = q.at(i)["class"].asString();
      if (qc != "mp2p_icp::QualityEvaluator_PairedRatio" && qc != "mp2p_icp_hip::QualityEvaluator_PairedRatio")
        throw std::runtime_error("quality evaluator '" + qc + "' is not available");
    }
  }
  return {icp, p};
}

void reload_plugin_switches() { molahip_host::reload_plugin_switches(); }
uint32_t plugin_switch_matched_points() { return molahip_host::plugin_switches().matched_points; }

}  // namespace mp2p_icp_hip
