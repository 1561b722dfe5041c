// LidarOdometry.h -- stand-alone LiDAR odometry driver over libmolahip.
//
// Restates the per-scan control flow of mola::LidarOdometry::onLidarImpl (module/src/LidarOdometry.cpp:622-1313,
// all "file:line" relative to /root/reference) so that a whole sequence can run on a box without the MOLA stack,
// configured by the reference's own pipeline file (pipelines/lidar3d-default.yaml / lidar3d-ndt.yaml):
//
//   [rigs] labelled observations -> sync window -> [device] sensor poses, per-sensor time offsets, merge   (:643-721)
//   raw scan -> [device] time-stamp adjust, decimate, range / box filters, de-skew      (yaml:267-350; :730-741)
//            -> constant-velocity guess                                                  (:808-811, 854-877)
//            -> [device] ICP with the twist-re-estimation hook loop                      (:919-1007)
//            -> goodness gate, motion-model update, trajectory                           (:1026-1045)
//            -> adaptive sigma                                                           (:1052-1064, 1437-1485)
//            -> key-frame decision, [device] local-map update                            (:1066-1118, 1160-1206)
// Localization in a saved map: saveLocalMaps() writes the local maps (molahip_host/local_map_file.h),
// params.local_map_updates.load_existing_local_map brings them back at initialize() / reset() (:465-470), initial_localization
// seeds the motion model at the first registration (:779-794), and relocalizeNearPose() -- the role of
// mola::Relocalization::relocalize_near_pose_pdf, whose body is a TODO in the reference (LidarOdometry.h:425-437,
// LidarOdometry.cpp:2222-2230) -- finds the pose in the map from a coarse one: a grid of candidates scored on the device in one
// launch (mh_score_poses), the best few refined by ICP.
//
// Key-frames of the session (params.simplemap; the role of the reference's simplemap, :1117-1138, 1209-1296): with
// simplemap.generate the scans that are far enough from the key-frames taken so far are kept on the host -- pose, covariance,
// twist and the layers their FilterMerge steps merge (not the raw observation: that layer is what a local-map key-frame merges,
// and it is 10-50 times smaller) -- and saved to a key-frame file (molahip_host/keyframe_file.h); build_session_maps() turns them
// into the maps of the WHOLE drive, one mh_map_insert_frames per map, in the format load_existing_local_map loads.  One
// deliberate difference: the reference stores the first scan even with generate: false (:817-824); here nothing is stored
// unless generate is on.
//
// Host code here is control logic only; every point touches the GPU through include/molahip.h.  What is NOT here:
// MOLA module plumbing, IMU/GNSS/wheel inputs (but for the gyroscope rate of gyro_deskew:, GyroDeskew.h), MRPT .simplemap
// serialisation, visualisation, ROS.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <regex>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/GyroDeskew.h"
#include "mola_lidar_odometry_hip/LiveMapCleaning.h"
#include "molahip_host/keyframe_file.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

using mp2p_icp_hip::Config;
using mp2p_icp_hip::CPose3D;
using mp2p_icp_hip::CPose3DPDFGaussianInf;
using mp2p_icp_hip::DeviceContext;
using mp2p_icp_hip::DevicePointCloud;
using mp2p_icp_hip::HashedVoxelPointCloud;
using mp2p_icp_hip::ICP;
using mp2p_icp_hip::Parameterizable;
using mp2p_icp_hip::ParameterSource;
using mp2p_icp_hip::TPose3D;

class OnlineLoopCloser;  // LoopClosure.h

struct Twist {
  double vx = 0, vy = 0, vz = 0, wx = 0, wy = 0, wz = 0;  // vehicle frame, the frame FilterDeskew integrates in
};

// Role of mola::NavStateFuse [U] (mola_navstate_fuse, not vendored; LidarOdometry.cpp:338, 810-811, 838, 1035-1038)
// restated as a constant-velocity model: the twist is the increment between the last two fused poses over their time
// difference (or `initial_twist`, yaml:137 / MOLA_INITIAL_VX of eval/cli_kitti.sh:25, while only one pose is known and
// that twist is not zero); the extrapolation composes the last pose with (Exp_SO3(w dt), v dt).  The upstream module is
// a sliding-window factor graph whose marginal also yields the prior information matrix that LidarOdometry.cpp:859-861
// hands to align(); here the prior is the simple propagation upstream used before the factor graph [U]: covariance
// of the last fused pose (the previous ICP result) + (sigma_random_walk_acceleration_{linear,angular} * dt)^2 on the
// diagonal (yaml:132-133), inverted.  It is switched by `motion_model_prior` (this implementation's own key; env
// MOLA_HIP_MOTION_MODEL_PRIOR in the -hip pipelines) and OFF by default: its strength relative to upstream's marginal
// is unverified, and a prior of the wrong strength pulls the solution towards the constant-velocity prediction (the
// synthetic drive that pulls away from rest at 13 m/s^2 ends 0.31 m off with it, 0.15 m without).  Poses older than
// max_time_to_use_velocity_model, or not newer than the last one, do not produce a twist.
class NavStateFuse {
 public:
  struct NavState {
    CPose3DPDFGaussianInf pose;  // cov_inv in the solver's tangent order [v; w]
    Twist twist;
  };
  double max_time_to_use_velocity_model = 2.0;  // [s] (yaml:130)
  double sigma_random_walk_acceleration_linear = 1.0;    // [m/s^2] (yaml:132)
  double sigma_random_walk_acceleration_angular = 10.0;  // [rad/s^2] (yaml:133)
  bool motion_model_prior = false;
  std::optional<Twist> initial_twist;
  void initialize(const Config& c);
  void reset();
  // cov: 6x6 row-major covariance of `pose` in (x,y,z,yaw,pitch,roll) (Results::optimal_tf.cov), or null = exact
  void fuse_pose(double t, const CPose3D& pose, const double* cov = nullptr);
  std::optional<NavState> estimated_navstate(double t) const;
  // a correction of the map frame (a loop closure): the last fused pose becomes delta (+) pose.  The twist is in the vehicle frame
  // and stays, as do the covariance and the times.
  void rebase(const CPose3D& delta);

 private:
  std::optional<CPose3D> last_pose_;
  double last_cov_[36] = {0};
  double last_t_ = 0;
  std::optional<Twist> twist_;
};

// Role of mola::SearchablePoseList [U] (mola_pose_list) with measure_from_last_kf_only = false: the key-frame poses,
// queried for the closest one (LidarOdometry.cpp:1066-1118).
class SearchablePoseList {
 public:
  bool empty() const { return poses_.empty(); }
  size_t size() const { return poses_.size(); }
  void insert(const CPose3D& p) { poses_.push_back(p); }
  // {is_first, p (-) closest key-frame}
  std::pair<bool, CPose3D> check(const CPose3D& p) const;
  void removeAllFartherThan(const CPose3D& p, double max_dist);
  void clear() { poses_.clear(); }

 private:
  std::vector<CPose3D> poses_;
};

// The key-frames of a session and the distance checker that decides them (state_.distance_checker_simplemap,
// LidarOdometry.cpp:1070-1071, 1117-1138), host logic only.  measure_from_last_kf_only: distances are measured from the last
// key-frame; otherwise from the closest of all (SearchablePoseList).  The rule, per scan that reached registration:
//   - the first scan (no ICP: it becomes the map) is a key-frame with points; the checker is not touched (:817-824);
//   - a scan with a good ICP is a key-frame iff it is the first pose in the checker, or its translation from the closest (or
//     last) key-frame exceeds min_translation [m], or its rotation exceeds min_rotation [deg]; it then enters the checker;
//   - with add_non_keyframes_too every other scan with a good ICP is stored without points;
//   - a scan with a bad ICP is not stored.
// Unlike the local-map rule neither a motion model nor local_map_updates.enabled is asked for.
class KeyFrameStore {
 public:
  struct Verdict {
    bool stored = false, keyframe = false;  // keyframe: stored with points
  };
  explicit KeyFrameStore(bool measure_from_last_kf_only = false) : last_only_(measure_from_last_kf_only) {}
  Verdict decide(bool first_scan, bool icp_good, const CPose3D& pose, double min_translation, double min_rotation_deg,
                 bool add_non_keyframes_too);
  void add(molahip_host::KeyFrame f) { set_.frames.push_back(std::move(f)); }
  // the frames (and the target maps they name); reset(): forget the checker and start from `initial` (a loaded file's content)
  const molahip_host::KeyFrameSet& set() const { return set_; }
  void setTargets(std::vector<molahip_host::KeyFrameTarget> maps) { set_.maps = std::move(maps); }
  // other poses for the stored frames (12 values each, one per frame: a loop closure's correction); the distance checker is
  // rebuilt from the new poses of the frames that had entered it
  void setPoses(const std::vector<double>& poses);
  void reset(const molahip_host::KeyFrameSet& initial = {});
  bool measureFromLastOnly() const { return last_only_; }

 private:
  bool last_only_;
  SearchablePoseList all_;
  std::optional<CPose3D> last_;
  std::vector<size_t> in_checker_;  // the frames whose poses entered the checker (decide() names the frame the next add() appends)
  molahip_host::KeyFrameSet set_;
};

// The key-frame layers that build target map `map_index` of a set, in frame order then step order, at the frames' poses; `keep`
// (optional) restricts the frames.  What build_session_maps() hands to insertFrames, and the driver when a loop closure rebuilds its
// local maps around the vehicle.  The pointers are into `set`.
std::vector<mp2p_icp_hip::PosedFrame> session_map_frames(const molahip_host::KeyFrameSet& set, size_t map_index,
                                                         const std::function<bool(const molahip_host::KeyFrame&)>& keep = nullptr);

// The maps of the whole drive from its key-frames: for every target map of the header a new map of the recorded class and
// parameters (mp2p_icp_hip::make_local_map), then ONE insertFrames of that map's layers in frame order, then step order;
// returned as the records saveLocalMaps() writes (remove_voxels_farther_than is the recorded one: what a run that loads the
// file and goes on mapping applies).  A header that names a CVoxelMap is refused: an occupancy map has no snapshot (recording
// such a plan is allowed, building from it is not).  max_points_per_pass: mh_map_insert_frames' (0 = the library's).
std::vector<molahip_host::LocalMapRecord> build_session_maps(const molahip_host::KeyFrameSet& frames, std::shared_ptr<DeviceContext> ctx = nullptr,
                                                             uint64_t max_points_per_pass = 0);
std::vector<molahip_host::LocalMapRecord> build_session_maps(const std::string& keyframe_file, std::shared_ptr<DeviceContext> ctx = nullptr,
                                                             uint64_t max_points_per_pass = 0);
// ... written as a version-1 local-map file (write_local_map_file): what load_existing_local_map loads
void build_session_map_file(const molahip_host::KeyFrameSet& frames, const std::string& local_map_file, std::shared_ptr<DeviceContext> ctx = nullptr,
                            uint64_t max_points_per_pass = 0);

// The pose rules of online_loop_closure: (LidarOdometry below), host logic only.  P: a scan's pose; S: the pose the key-frame store
// holds for a stored frame at that time; C: a frame's corrected pose.
CPose3D loop_raw_pose(const CPose3D& raw_prev, const CPose3D& P, const CPose3D& S_prev);  // raw_k = raw_{k-1} (+) (P_k (-) S_{k-1}); P_k itself while S_{k-1} == raw_{k-1}
CPose3D loop_correction(const CPose3D& C, const CPose3D& P);                              // delta = C (+) P^-1: delta (+) P = C
CPose3D trajectory_anchor(const CPose3D& P, const CPose3D& S);                            // rel = P (-) S
CPose3D trajectory_corrected(const CPose3D& C, const CPose3D& rel);                       // C (+) rel

// The grouping rule of a multi-LiDAR rig (LidarOdometry.cpp:664-689, 702-713), host logic only: the latest observation of
// every label waits until `lidar_count` labels are present; the group is then the waiting observations within
// `max_time_offset` of the one that completed it, in byte-wise label order (the order of the reference's std::map), and the
// waiting set is emptied.  The reference time is the stamp of the FIRST KEPT observation in that order, not the first to arrive.
// lidar_count <= 1: every observation is a group of its own.
class SensorSync {
 public:
  struct Group {
    std::vector<std::string> labels;     // kept, in merge order
    std::vector<double> stamps, dts;     // their time stamps; dts[k] = stamps[k] - stamps[0] (each source's SENSOR_TIME_OFFSET)
    std::vector<std::string> discarded;  // waiting observations outside the window
  };
  explicit SensorSync(uint32_t lidar_count = 1, double max_time_offset = 25e-3) : lidar_count_(lidar_count), max_time_offset_(max_time_offset) {}
  // a newer observation of a label replaces the one that waits
  std::optional<Group> push(const std::string& label, double stamp);
  void clear() { waiting_.clear(); }
  std::vector<std::string> waiting() const;
  uint32_t lidarCount() const { return lidar_count_; }
  double maxTimeOffset() const { return max_time_offset_; }

 private:
  uint32_t lidar_count_;
  double max_time_offset_;
  std::map<std::string, double> waiting_;
};

// The candidate poses of a relocalization around `mean` with covariance `cov` (6x6 row-major, (x, y, z, yaw, pitch, roll)
// order): a grid over x, y and yaw; z, pitch and roll are the mean's.  Per axis n = 2 * ceil(sigmas * sigma / step) + 1 nodes at
// (i - (n - 1) / 2) * step, sigma = sqrt of the axis' diagonal entry; the offsets are added to the mean's TPose3D fields (map
// frame); enumeration order x outer, y middle, yaw inner.  More than max_candidates nodes: std::runtime_error (coarsen the steps).
std::vector<TPose3D> relocalization_grid(const TPose3D& mean, const double cov[36], double step_xy, double step_yaw_rad,
                                         double sigmas = 3.0, size_t max_candidates = 65536);
// ... whether that grid stays within max_candidates (the same count, without making the poses)
bool relocalization_grid_fits(const double cov[36], double step_xy, double step_yaw_rad, double sigmas = 3.0, size_t max_candidates = 65536);

// Steps 2-4 of LidarOdometry::relocalizeNearPose on their own (the driver calls this; so does a loop closure's verification,
// LoopClosure.h): ONE mh_score_poses of `local_layer` of pcLocal (a DevicePointCloud) against `global_layer` of pcGlobal (a device
// map) over all candidates at score_threshold; rank by (n_paired descending, cost ascending, index ascending), keep refine_top_k;
// icp.align from each kept candidate with hooks cleared and no prior, one after another; the winner has the highest quality, ties
// go to the better rank.  The ICP's dynamic variables are the caller's business.  `seconds` (optional): wall time is added to its
// entries "score" and "refine".
struct RelocalizationRefinement {
  std::vector<uint32_t> ranks;           // the candidates refined, in rank order
  std::vector<mh_pose_score> scores;     // ... and their scores
  bool have = false;                     // false: no candidate at all
  mp2p_icp_hip::Results best;            // the winner's alignment
};
RelocalizationRefinement score_rank_refine(ICP& icp, const mp2p_icp_hip::Parameters& icp_params, const mp2p_icp_hip::metric_map_t& pcLocal,
                                           const mp2p_icp_hip::metric_map_t& pcGlobal, const std::string& global_layer, const std::string& local_layer,
                                           const std::vector<TPose3D>& candidates, double score_threshold, uint32_t refine_top_k,
                                           std::map<std::string, double>* seconds = nullptr);

// Place recognition over the key-frames of a session (include/molahip.h, mh_place_*): an mh_place_db of the polar height
// descriptors of the frames' first stored layer (layers[0]: the input layer of the first FilterMerge step, vehicle frame) and the
// frame every descriptor belongs to.  Descriptors are recomputed from the stored layers; the key-frame file does not hold them.
class PlaceIndex {
 public:
  struct Match {
    uint32_t frame = 0, shift = 0, dist = 0;  // index into the KeyFrameSet's frames; mh_place_match of its descriptor
  };
  explicit PlaceIndex(const mh_place_params& params, std::shared_ptr<DeviceContext> ctx = nullptr);
  ~PlaceIndex();
  PlaceIndex(const PlaceIndex&) = delete;
  PlaceIndex& operator=(const PlaceIndex&) = delete;
  // appends the frames from index `first` on that have points (a non-empty layers[0]) in ONE mh_place_db_add_frames; returns
  // how many were appended
  size_t addKeyFrames(const molahip_host::KeyFrameSet& set, size_t first = 0);
  // every stored descriptor against the layer's, ranked by (dist ascending, frame ascending)
  std::vector<Match> query(const DevicePointCloud& layer) const;
  std::vector<uint8_t> describe(const DevicePointCloud& layer) const;  // n_rings * n_sectors bytes, desc[ring * S + sector]
  size_t size() const { return frame_of_.size(); }
  const mh_place_params& params() const { return params_; }

 private:
  std::shared_ptr<DeviceContext> ctx_;
  mh_place_params params_;
  mh_place_db* db_ = nullptr;
  std::vector<uint32_t> frame_of_;
};

// The optional top-level lost_recovery: block (this implementation's own key): what LidarOdometry does once its own judgement of
// the alignments says that the vehicle is lost.  An absent block and enabled: false leave the driver as it is without the block.
struct LostRecoveryOptions {
  bool enabled = false;
  uint32_t bad_scans_to_lost = 3;               // consecutive rejected alignments that make the driver LOST
  std::string method = "near_then_keyframes";   // near | keyframes | near_then_keyframes
  double near_sigma_xy = 3.0;                   // [m]   the covariance of a `near` attempt around the last good pose: x, y ...
  double near_sigma_yaw_deg = 15.0;             // [deg] ... and yaw; the other entries are zero
  uint32_t retry_every_n_scans = 5;             // scans from one attempt to the next while LOST
  uint32_t max_attempts = 0;                    // per loss; 0: no limit
  bool needsKeyFrames() const { return method != "near"; }
  // out of range: std::runtime_error starting "lost_recovery: <key>"
  static LostRecoveryOptions FromConfig(const Config& pipeline);
  void validate() const;
};

// The state machine of lost_recovery: (LidarOdometry below), host logic only: the driver tells it what happened to a scan and does
// what it answers.  Per scan that reaches registration, in this order:
//   1. lost() is the state the scan arrived in;
//   2. a pending relocalization request was served -> served(succeeded): the driver's own request counts as an attempt; success of
//      anyone's request is TRACKING with the streaks at zero; a failed own request is to be cleared (the answer) and the next one
//      is due retry_every_n_scans scans after this one;
//   3. the alignment ran and the scan did not restart the map -> gate(icp_good): a rejected one extends the bad streak, and at
//      bad_scans_to_lost the driver is LOST (the first attempt is due at once); a good one ends the bad streak, and while LOST
//      bad_scans_to_lost good ones in a row are TRACKING again;
//   4. due(request_pending, near_fits) -> the attempt to place now for the NEXT observation (0 none, 1 near, 2 keyframes): only while
//      LOST, no request of anyone pending, the retry count run down and max_attempts not reached; with near_then_keyframes the first
//      attempt of a loss is `near`, every later one `keyframes`.  A `near` attempt whose candidate grid would exceed
//      relocalization.max_candidates (near_fits false) is SKIPPED: no request is placed and no device work done, so it is no
//      attempt -- neither attempts() nor max_attempts count it, skipped() does; near_then_keyframes goes on to `keyframes` at
//      once, method near waits retry_every_n_scans scans and looks again.  placed(kind) after the request was made;
//      callerRequested() when the caller made one (it replaces the driver's own).
class LostRecovery {
 public:
  struct Fields {  // what a ScanRecord shows of this
    bool lost = false, recovery_succeeded = false;
    uint32_t recovery_attempt = 0, bad_streak = 0;
  };
  explicit LostRecovery(const LostRecoveryOptions& o = LostRecoveryOptions()) : o_(o) {}
  void reset() { *this = LostRecovery(o_); }
  bool lost() const { return lost_; }
  uint32_t badStreak() const { return bad_streak_; }
  uint32_t ownPending() const { return own_pending_; }
  uint32_t timesLost() const { return times_lost_; }
  uint32_t attempts() const { return attempts_; }
  uint32_t timesRecovered() const { return times_recovered_; }
  bool gaveUp() const { return lost_ && o_.max_attempts != 0 && attempts_this_loss_ >= o_.max_attempts; }
  void callerRequested() { own_pending_ = 0; }
  bool served(bool succeeded, Fields& f);   // true: clear the request (the driver's own, failed)
  void gate(bool icp_good, Fields& f);
  uint32_t due(bool request_pending, bool near_fits = true);
  uint32_t skipped() const { return skipped_; }  // `near` attempts skipped (no attempts: attempts() does not count them)
  void placed(uint32_t kind) { own_pending_ = kind; }
  const LostRecoveryOptions& options() const { return o_; }

 private:
  LostRecoveryOptions o_;
  bool lost_ = false, near_done_ = false;  // near_done_: this loss has had its `near` turn (near_then_keyframes)
  uint32_t bad_streak_ = 0, good_streak_ = 0, own_pending_ = 0, wait_ = 0, attempts_this_loss_ = 0;
  uint32_t times_lost_ = 0, attempts_ = 0, times_recovered_ = 0, skipped_ = 0;
};

class LidarOdometry {
 public:
  // the params: block of the pipeline file (yaml:6-122); formulas are re-evaluated every scan
  struct Params : public Parameterizable {
    double min_time_between_scans = 0.2;
    double max_sensor_range_filter_coefficient = 0.999;
    double absolute_minimum_sensor_range = 5.0;
    bool optimize_twist = false;
    double optimize_twist_rerun_min_trans = 0.1, optimize_twist_rerun_min_rot_deg = 0.5;
    size_t optimize_twist_max_corrections = 8;
    bool local_map_updates_enabled = true;
    double min_translation_between_keyframes = 1.0, min_rotation_between_keyframes = 30.0;  // [m] [deg] formulas
    double max_distance_to_keep_keyframes = 0.0;                                            // formula
    uint32_t check_for_removal_every_n = 100;
    double min_icp_goodness = 0.4;
    bool adaptive_threshold_enabled = true;
    double initial_sigma = 0.5, min_motion = 0.1, maximum_sigma = 5.0, kp = 5.0, alpha = 0.99;
    bool validity_check_enabled = false;
    uint32_t validity_minimum_point_count = 1000;
    uint32_t lidar_count = 1;        // multiple_lidars.lidar_count (reference LidarOdometry.h:152)
    double max_time_offset = 25e-3;  // multiple_lidars.max_time_offset [s] (:156)
    std::vector<std::string> lidar_sensor_labels;  // regular expressions, std::regex_match (:261-275, 576-577); empty: every label
    // local_map_updates.load_existing_local_map (MOLA_LOAD_MM, yaml:40; :465-470): a file written by saveLocalMaps().  Non-empty:
    // the local maps are created from the FILE's parameters and restored at initialize() and again by reset(); the first
    // observation is then registered by ICP (no "first scan" entry).  With mapping enabled the key-frame list starts empty, so
    // the first good alignment with a motion model is a key-frame merged into the loaded map (multi-session mapping).  The rule
    // "bad ICP while the trajectory holds one pose: clear the map and start again" (:1148-1158) is kept and CAN discard a loaded map.
    std::string load_existing_local_map;
    // the simplemap: block (reference LidarOdometry.h:280-332), same keys.  The two min_* are formulas like local_map_updates'.
    // load_existing_simple_map names a key-frame file (molahip_host/keyframe_file.h) whose frames the store starts with.  New
    // frames go under the file's header: its map names are held against the pipeline's at initialize(), its classes and
    // mh_map_params when the maps exist (the scan that makes them throws if they differ); its remove_voxels_farther_than stays;
    // generate_lazy_load_scan_files: true is refused at initialize(); save_gnss_max_age is read and ignored (no GNSS input).
    struct SimpleMapOptions {
      bool generate = false;
      double min_translation_between_keyframes = 1.0, min_rotation_between_keyframes = 30.0;  // [m] [deg] formulas
      bool measure_from_last_kf_only = false, add_non_keyframes_too = false, generate_lazy_load_scan_files = false;
      double save_gnss_max_age = 1.0;
      std::string save_final_map_to_file, load_existing_simple_map;
    } simplemap;
    void load_from(const Config& c);
  };
  // the initial_localization: block of the pipeline file (yaml:147-151; :779-794).  enabled: at the first observation that
  // reaches registration the fixed pose is fused into the motion model at t - 0.2 and t - 0.1 (once), so that registration
  // starts there with a zero twist.  Only InitLocalization::FixedPose exists here (no GNSS input): anything else is refused at
  // initialize().  relocalize_sigmas: [sigma_x [m], sigma_y [m], sigma_yaw [deg]] is this implementation's extension: the first
  // observation is then served by relocalizeNearPose() around fixed_initial_pose instead of the plain seed.
  struct InitialLocalization {
    bool enabled = false;
    std::string method = "InitLocalization::FixedPose";
    TPose3D fixed_initial_pose;
    bool relocalize = false;
    double relocalize_sigmas[3] = {0, 0, 0};
  };
  // the relocalization: block (this implementation's own key, as motion_model_prior is)
  struct RelocalizationOptions {
    std::string score_threshold;  // [m] formula over the dynamic variables; empty: 0.5 x the searched map's voxel size
    double step_xy = 0;           // [m] 0: the score threshold
    double step_yaw_deg = 3.0;
    double sigmas = 3.0;
    uint32_t refine_top_k = 4;
    uint32_t max_candidates = 65536;
    // relocalizeInKeyFrames: the descriptor (mh_place_params), the ranked frames kept, and the spread searched around each
    uint32_t place_rings = 20, place_sectors = 64;
    double place_min_range = 1.0, place_max_range = 80.0, place_z_min = -3.0, place_z_max = 27.0;
    uint32_t place_top_k = 4;
    double place_sigma_xy = 1.0;          // [m]
    double place_sigma_yaw_deg = 5.625;   // one sector of the default descriptor
  };

  // one line of the per-scan log (what the reference spreads over debug traces / the parameter source)
  struct ScanRecord {
    double timestamp = 0;
    bool dropped = false, first_scan = false, icp_run = false, icp_good = false, had_motion_model = false,
         map_updated = false, restarted = false;
    CPose3D pose;             // state_.last_lidar_pose after this scan
    CPose3D init_guess;       // what ICP started from
    double goodness = 0, sigma = 0, estimated_sensor_max_range = 0, instantaneous_sensor_max_range = 0;
    uint32_t icp_iterations = 0, twist_corrections = 0, align_calls = 0;
    int termination = 0;
    // n_map_points / n_map_voxels: the map AFTER this scan.  In the reference returned by onLidar*() they are still 0 for a
    // key-frame scan (and for the scans up to the next read-back): the update is asynchronous; records() fills them in.
    uint64_t n_raw = 0, n_for_map = 0, n_for_icp = 0, n_map_points = 0, n_map_voxels = 0;
    Twist twist;              // twist used for the (last) de-skew of this scan
    double decim_map_resolution = 0, decim_icp_resolution = 0, map_voxel_size = 0;
    // general filter chains (not the default one, whose record leaves it empty): points of every observation layer handed to
    // ICP, by name.  There n_for_map = points the FilterMerge steps offered to the maps, n_for_icp = points of all those layers.
    // All three describe the layers that were finally aligned and merged: after the last re-run of the 2nd pass that the twist
    // hook asked for (a 2nd pass that filters after its de-skew can change them; LidarOdometry.cpp:973-1004, 1158-1206).
    std::map<std::string, uint64_t> layer_sizes;
    // labelled observations (onLidarFrom): `ignored` = the label matches none of lidar_sensor_labels; `waiting` = uploaded, the
    // group is not complete yet (no trajectory entry, the pose unchanged).  n_sensors = sources merged into this scan (1 on the
    // unlabelled entry points), sensor_labels = their labels in merge order; n_raw is the merged count.
    bool waiting = false, ignored = false;
    uint32_t n_sensors = 1;
    std::vector<std::string> sensor_labels;
    // a relocalization request served at this scan (relocalizeNearPose): candidates scored, the best candidate's accepted
    // points, the winner's ICP quality, the candidate indices that were refined (in rank order); relocalized = accepted
    bool relocalization_tried = false, relocalized = false;
    uint32_t reloc_candidates = 0, reloc_best_n_paired = 0;
    double reloc_best_quality = 0;
    std::vector<uint32_t> reloc_ranks;
    // ... a relocalizeInKeyFrames request: the key-frames kept by the place search in rank order (indices into keyFrames()),
    // their column shifts and descriptor distances
    bool place_tried = false;
    std::vector<uint32_t> place_frames, place_shifts, place_dists;
    // params.simplemap.generate: this scan is stored in the key-frame store (simplemap_frame), with its points (simplemap_keyframe)
    bool simplemap_keyframe = false, simplemap_frame = false;
    // online_loop_closure: this scan's stored frame went to the loop closer, which verified loop_pairs = (i, j, quality, accepted)
    // for it (loop_tried) and accepted one (loop_closed).  With correct_driver the closure moved the map frame by delta: `pose` is
    // the corrected one, loop_correction_trans [m] / loop_correction_rot [rad] are delta's norms and loop_rebuilt_frames the
    // key-frames the local maps were rebuilt from.
    bool loop_tried = false, loop_closed = false;
    struct LoopPairRecord {
      uint32_t i = 0, j = 0;
      double quality = 0;
      bool accepted = false;
    };
    std::vector<LoopPairRecord> loop_pairs;
    double loop_correction_trans = 0, loop_correction_rot = 0;
    uint32_t loop_rebuilt_frames = 0;
    // lost_recovery: the driver was LOST when this scan arrived (lost); the request this scan served was the driver's own
    // (recovery_attempt: 0 none, 1 near, 2 keyframes) and was accepted (recovery_succeeded); bad_streak = rejected alignments in a
    // row up to and including this scan.  recovery_gave_up: when this scan ended the driver was LOST with max_attempts used up (it
    // places no further request; a caller's request or bad_scans_to_lost good alignments still bring it back).
    bool lost = false;
    uint32_t recovery_attempt = 0;
    bool recovery_succeeded = false;
    uint32_t bad_streak = 0;
    bool recovery_gave_up = false;
    // online_map_cleaning: this scan's local map update was followed by an erasing of the target maps (LiveMapCleaning.h);
    // n_map_points / n_map_voxels are then the counts AFTER the erasing
    bool map_cleaned = false;
    // gyro_deskew: this scan's 2nd pass de-skewed with a motion table of gyro_segments segments cut from the gyro samples
    // (false with the block enabled: the samples did not cover the sweep and the constant twist was used)
    bool gyro_deskew = false;
    uint32_t gyro_segments = 0;
  };

  // ctx == nullptr: the process-wide default device context, taken at initialize()
  explicit LidarOdometry(std::shared_ptr<DeviceContext> ctx = nullptr);
  ~LidarOdometry();

  // cfg = the whole pipeline file (keys: params, navstate_fuse_params, icp_settings_with_vel[, icp_settings_without_vel],
  // localmap_generator, observations_filter_adjust_timestamps, observations_filter_1st_pass, observations_filter_2nd_pass,
  // insert_observation_into_local_map).  Throws std::runtime_error on a filter chain the device path does not implement.
  void initialize(const Config& cfg);
  void reset();

  // One LiDAR observation: points in the vehicle frame, optional per-point time stamps [s] relative to `timestamp`.
  // Returns the record of this scan (also appended to records()).
  const ScanRecord& onLidar(double timestamp, const float* x, const float* y, const float* z, const float* t, size_t n);
  // The same for raw interleaved records as sensors and data sets deliver them (KITTI velodyne .bin: point_step 16,
  // offsets 0/4/8; PointCloud2: its own): the bytes go to the device as they are and are split into channels there
  // (the job of observations_generator, lidar3d-default.yaml:250-262).  Time stamps: float32 field at off_t (>= 0), or
  // the separate array `t` (may be nullptr).  Intensity: float32 field at off_i (>= 0), read only when the pipeline holds an
  // intensity filter (setIntensityInput); such a pipeline rejects a scan without it.
  const ScanRecord& onLidarInterleaved(double timestamp, const void* data, size_t n, size_t point_step, size_t off_x,
                                       size_t off_y, size_t off_z, long long off_t = -1, const float* t = nullptr,
                                       long long off_i = -1);

  // One observation of a labelled sensor of a rig (params.multiple_lidars, params.lidar_sensor_labels), the points in the
  // SENSOR frame: `sensor_pose` is the sensor on the vehicle (12 doubles, row-major 3x4; null = identity).  Restates
  // LidarOdometry.cpp:643-721 and :759-763 in their order: label filter -> minimum time between scans per label -> upload
  // into a device layer kept per label (the caller's buffer is borrowed for the call only; page-locked input as
  // setInputPinned says) -> first-call sensor-range estimate from this one observation in the vehicle frame -> wait until
  // lidar_count labels are present (SensorSync) -> ONE mh_scan_merge_sensors of the kept observations into 'raw' (sensor poses,
  // FilterAdjustTimestamps per source with SENSOR_TIME_OFFSET = its stamp minus the first kept one's) -> the rest of onLidar at
  // the triggering observation's time stamp.  With lidar_count 1 it is the same flow with a group of one: a single LiDAR with a
  // mounting pose.  On a rig (lidar_count > 1) onLidar, onLidarInterleaved and prefetch* throw; prefetch* also throws once a
  // labelled observation has been received (no prefetch overlap for rigs).
  const ScanRecord& onLidarFrom(const std::string& sensor_label, const double* sensor_pose, double timestamp, const void* data,
                                size_t n, size_t point_step, size_t off_x, size_t off_y, size_t off_z, long long off_t = -1,
                                const float* t = nullptr, long long off_i = -1);

  // One depth-image observation, for a pipeline whose observations_generator is a GeneratorEdgesFromRangeImage (rgbd.yaml):
  // `range` is row-major camera.rows x camera.cols, 0 = no return; `camera` holds the intrinsics, the range encoding and the
  // sensor's pose on the vehicle (include/molahip.h, mh_range_image_params); its row_window_length and score_threshold are
  // overwritten from the pipeline.  With setInputPinned(true) `range` is page-locked and uploaded asynchronously.  A pipeline
  // that takes point clouds throws here, and onLidar* throws on a depth-image pipeline (std::runtime_error, naming the other).
  const ScanRecord& onDepthImage(double timestamp, const uint16_t* range, const mh_range_image_params& camera);

  // Off-line replay (data sets, eval/cli_kitti.sh): announce the NEXT observation before calling onLidar* for the
  // current one.  Its upload and first filter pass then run on a second stream of the same device, in a worker thread,
  // while the current scan is in its ICP loop; the next onLidar* call (same buffer, same layout) picks the result up.
  // The buffers must stay valid until that call.  Results are identical to the sequential flow: the first pass only
  // depends on the sensor-range estimate, which is final before ICP starts; if any filter parameter turns out
  // different when the scan is really due, the prepared layers are dropped and the pass runs again.
  // several sequences in one process: the ICP of this instance joins the others' in one lock-step batch per round
  // (mp2p_icp_hip::AlignBatcher); call after initialize(), drive every instance from its own host thread
  void setAlignBatcher(std::shared_ptr<mp2p_icp_hip::AlignBatcher> b);
  void prefetchInterleaved(const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y, size_t off_z,
                           long long off_t = -1, const float* t = nullptr, long long off_i = -1);
  // Before initialize(): the observations carry a float32 intensity (onLidarInterleaved's off_i).  Only then does a general
  // plan accept FilterNormalizeIntensity / FilterByIntensity; without it initialize() rejects them.
  void setIntensityInput(bool on) { intensity_input_ = on; }
  void prefetch(const float* x, const float* y, const float* z, const float* t, size_t n);

  // (n_map_points / n_map_voxels of the records since the last key-frame are read back from the device lazily: here, and
  // before the next key-frame update -- by then the update has long finished, so the replay itself never waits for it)
  const std::vector<ScanRecord>& records() const { resolve_map_counts(); return records_; }
  const std::vector<std::pair<double, CPose3D>>& estimatedTrajectory() const { return trajectory_; }
  // TUM format "t x y z qx qy qz qw" (estimated_trajectory.output_file, yaml:79-81; eval/cli_kitti.sh:41-50)
  void saveTrajectoryTUM(const std::string& path) const;
  // The trajectory as the loop closures so far correct it: every entry hangs on the last stored key-frame at or before it by the
  // relative pose it had when it was made, and follows that frame's corrected pose (entries before the first stored frame stay).
  // estimatedTrajectory() bit for bit while no loop has been closed; estimatedTrajectory() itself keeps what was estimated at the time.
  std::vector<std::pair<double, CPose3D>> correctedTrajectory() const;
  void saveCorrectedTrajectoryTUM(const std::string& path) const;
  // online_loop_closure: (LoopClosure.h) -- enabled: every stored key-frame goes to an OnlineLoopCloser with its RAW pose, raw_k =
  // raw_{k-1} (+) (P_k (-) S_{k-1}): P_k the scan's pose, S_{k-1} the pose the store holds for the previous frame at that time; a
  // load_existing_simple_map file's frames go first with their file poses.  With correct_driver an accepted closure is fed back
  // inside the same onLidar* call, after the scan's own map update: the store's poses become the corrected ones, the last pose and
  // the motion model move by delta = C_i (+) P_i^-1, and every local map is cleared and rebuilt by one insertFrames from the stored
  // key-frames within its recorded remove_voxels_farther_than of the vehicle (0: all).  initialize() demands simplemap.generate and
  // refuses a CVoxelMap plan and an ICP block close_loops() would refuse; setAlignBatcher() throws.
  // loopCloser(): null when disabled or before the first stored frame; it reads the layers of this object's key-frame store (no second
  // copy of the session's points), so it is to be used while this object lives.  rawKeyFrames(): the set on which close_loops()
  // reproduces the run.
  std::shared_ptr<const OnlineLoopCloser> loopCloser() const { return loop_closer_; }
  molahip_host::KeyFrameSet rawKeyFrames() const;
  const Params& params() const { return params_; }
  const InitialLocalization& initialLocalization() const { return init_loc_; }
  const RelocalizationOptions& relocalizationOptions() const { return reloc_opts_; }
  // Every local map of the plan, by name, into one file (molahip_host/local_map_file.h); throws before the first key-frame
  // (no map yet) and for a plan with a CVoxelMap (an occupancy map has no snapshot).
  void saveLocalMaps(const std::string& path) const;
  // The key-frames stored so far (empty unless params.simplemap.generate, or a load_existing_simple_map file was given), and
  // their file.  The destructor writes params.simplemap.save_final_map_to_file when that is set and generate is on.
  const molahip_host::KeyFrameSet& keyFrames() const { return kf_store_.set(); }
  void saveKeyFrames(const std::string& path) const;
  // The role of mola::Relocalization::relocalize_near_pose_pdf: `mean` with covariance `cov` (6x6 row-major, (x, y, z, yaw, pitch,
  // roll)) is where the vehicle is believed to be in the map frame.  The request is served by the next observation that reaches
  // registration with a non-empty map, after its filter passes and before the motion-model query:
  //   1. candidates: relocalization_grid over x, y, yaw (relocalization.step_xy / step_yaw_deg / sigmas); more than
  //      max_candidates makes THIS call throw (when the map whose voxel sizes the defaults is not there yet: the serving scan);
  //   2. one mh_score_poses of the (global, local) layers of the first pointLayerMatches entry of the first enabled
  //      Matcher_Points_DistanceThreshold of the no-motion-model ICP block, at relocalization.score_threshold;
  //   3. rank by (n_paired descending, cost ascending, index ascending), keep refine_top_k;
  //   4. align from each kept candidate with the NoMotionModel ICP, no prior, hooks cleared, one after another; the winner has
  //      the highest quality, ties go to the better rank;
  //   5. quality >= min_icp_goodness: the motion model is reset and seeded with the winner's pose as initial_localization does,
  //      the last pose is set, the request is cleared and the scan's normal registration runs from there; otherwise the request
  //      stays pending for the next observation and the scan proceeds as it would have.
  // At relocalization time the twist is unknown: the layers were de-skewed with the current twist variables, which are zero
  // after a reset.  With an AlignBatcher set this throws: the batch protocol has no slot for extra alignments of one member.
  void relocalizeNearPose(const CPose3D& mean, const double cov[36]);
  // The same without a coarse pose: place recognition over the stored key-frames supplies it.  Preconditions and failure path
  // are relocalizeNearPose's.  The serving scan
  //   1. brings a PlaceIndex (relocalization.place_rings ... place_z_max) up to date with the key-frame store (keyFrames(): a
  //      load_existing_simple_map file's frames and those recorded since) and describes the input layer of the first FilterMerge
  //      step as this scan's passes left it -- the role layers[0] has in a key-frame; a store without a frame with points
  //      throws and names load_existing_simple_map;
  //   2. searches and keeps the first place_top_k frames, ranked by (dist ascending, frame ascending);
  //   3. per kept frame: mean = frame pose (+) Rz(-shift * 2 pi / place_sectors), candidates = relocalization_grid(mean,
  //      diag(place_sigma_xy^2, place_sigma_xy^2, ., place_sigma_yaw^2, ., .)) with the steps, sigmas and max_candidates above;
  //      the lists are concatenated in rank order and their total counts against max_candidates;
  //   4. runs steps 2-5 of relocalizeNearPose on the concatenated list.
  void relocalizeInKeyFrames();
  bool relocalizationPending() const { return reloc_request_.has_value(); }
  // lost_recovery: (LostRecoveryOptions, LostRecovery above) -- enabled: the driver judges by its own alignments whether it is lost and
  // then places the requests above itself.  All of it is host logic inside onLidar* / onLidarFrom / onDepthImage, after the gate
  // that sets icp_good:
  //   1. TRACKING -> LOST: bad_scans_to_lost scans in a row with icp_run && !icp_good (a scan that restarted the map neither counts
  //      nor breaks the run); the pose of that moment -- the last good one -- is remembered;
  //   2. the scan that makes the driver LOST places the first request; the NEXT observation serves it, as it serves a caller's.
  //      near: relocalizeNearPose(remembered pose, diag(near_sigma_xy^2, near_sigma_xy^2, ., near_sigma_yaw^2, ., .));
  //      keyframes: relocalizeInKeyFrames(); near_then_keyframes: the first attempt of a loss is near, every later one keyframes;
  //   3. a failed attempt clears the driver's own request (a caller's stays pending, as before); the next one is placed so that it
  //      is served retry_every_n_scans scans after the failed one; after max_attempts (not 0) attempts of one loss none is placed
  //      (recoveryGaveUp(), recovery_gave_up of the records).  An own request that cannot be served at all -- the key-frame store
  //      holds no frame with points, the grids around the kept key-frames exceed relocalization.max_candidates, the scored layers
  //      are not among the scan's -- would throw out of onLidar* on every scan with nobody to withdraw it: it is a failed attempt
  //      like any other (the record shows the attempt and no search), and lastRecoveryError() keeps what was thrown.  A caller's
  //      request throws as before.  A `near` attempt whose grid would exceed max_candidates is not placed at all (LostRecovery);
  //   4. a caller's request takes precedence: while one is pending the driver places none, and a caller's request replaces the
  //      driver's own; if it succeeds the driver is TRACKING;
  //   5. while LOST an alignment that passes min_icp_goodness moves the pose, the motion model and the trajectory as before, but
  //      neither the local maps (nor their key-frame list) nor the key-frame store take the scan;
  //   6. LOST -> TRACKING: an accepted request (step 5 of relocalizeNearPose: the serving scan's registration runs from the
  //      found pose and is trusted again), or bad_scans_to_lost good alignments in a row (the last of them is trusted again),
  //      whichever comes first; the streaks are zero then.
  // initialize() refuses, naming lost_recovery: -- a method that needs key-frames without simplemap.generate or
  // load_existing_simple_map; online_loop_closure: enabled (its raw chain has no rule for a jump); an AlignBatcher (setAlignBatcher
  // refuses too, both in the words of relocalizeInKeyFrames' refusal); and whatever relocalizeNearPose / relocalizeInKeyFrames
  // refuse of the plan.  reset() is TRACKING, all counts zero.
  const LostRecoveryOptions& lostRecoveryOptions() const { return lost_.options(); }
  bool isLost() const { return lost_.lost(); }
  uint32_t timesLost() const { return lost_.timesLost(); }
  uint32_t recoveryAttempts() const { return lost_.attempts(); }
  uint32_t timesRecovered() const { return lost_.timesRecovered(); }
  bool recoveryGaveUp() const { return lost_.gaveUp(); }                      // LOST, and max_attempts used up
  const std::string& lastRecoveryError() const { return recovery_error_; }  // what the last own request that could not be served threw
  // online_map_cleaning: (LiveMapCleaning.h) -- enabled: every local map update is followed, inside the same onLidar* call and
  // after all of its insertPointCloud calls, by the rule of LiveMapCleaner on the target maps: the view of view_layer's cloud into
  // the ring, then (every every_n_updates updates) one mh_map_erase_seen_through per target map -- all queued on the device.
  // Whatever clears the maps (the restart after a bad first alignment, reset()) empties the ring.  Key-frames go into the
  // key-frame store as recorded.  initialize() refuses, naming online_map_cleaning: -- a target that is a CVoxelMap or not a map
  // of the plan, a view_layer the plan does not make, online_loop_closure: with correct_driver (its rebuild from the key-frames
  // would bring the erased points back), an AlignBatcher (setAlignBatcher refuses too).
  const OnlineMapCleaningOptions& onlineMapCleaningOptions() const { return live_opts_; }
  uint64_t mapPointsErased() const;  // points erased from the target maps since they were created (waits for the device)
  // gyro_deskew: (GyroDeskew.h) -- enabled: onGyro() feeds a GyroBuffer (any time, any thread that also calls onLidar*: not
  // concurrently with them); every scan that reaches its 2nd pass asks build_motion_table(buffer, its time stamp, the options)
  // ONCE for the rotations of its sweep, and both the default plan's de-skew pair and every FilterDeskew step of a general plan
  // then call mh_scan_deskew_motion[_pair] with them and the current vx, vy, vz -- the twist hook re-runs the pass with a new v
  // and the same rotations (wx, wy, wz are not read).  A scan whose sweep the samples do not cover is de-skewed with the constant
  // twist as without the block (ScanRecord::gyro_deskew says which).  skip_deskew wins over the block.  initialize() refuses,
  // naming gyro_deskew: -- a depth-image plan (no time stamps to de-skew by) and an AlignBatcher (setAlignBatcher refuses too).
  // With the block absent or disabled onGyro() ignores the sample.  Call it after initialize(); reset() empties the buffer.
  void onGyro(double t, const double w[3]);
  const GyroDeskewOptions& gyroDeskewOptions() const { return gyro_opts_; }
  uint64_t scansGyroDeskewed() const { return scans_gyro_deskewed_; }
  uint64_t gyroSamplesDropped() const { return gyro_buf_.dropped(); }
  std::shared_ptr<HashedVoxelPointCloud> localMap() const { return local_map_; }
  // points of every local map by name (general plans: one per localmap_generator entry; 0 before the first key-frame)
  std::map<std::string, uint64_t> localMapSizes() const;
  // Debug accessors for tests (they wait for the device and copy to the host: not for timed paths).
  // Every local map by name: stored points, occupied voxels, voxel size (zeros before the first key-frame).
  struct MapStats {
    uint64_t n_points = 0, n_voxels = 0;
    double voxel_size = 0;
  };
  std::map<std::string, MapStats> localMapStats() const;
  // The class of every local map object by name: "HashedVoxelPointCloud" (also an NDT map, which is one with plane
  // statistics), "CVoxelMap" or "SparseTreesPointCloud" ("" before the first key-frame).
  std::map<std::string, std::string> localMapClasses() const;
  // An observation layer of the last scan of a general plan, as the last run of its filter left it (a layer that a
  // FilterDeleteLayer removed keeps its content until the next scan writes it): coordinates, time stamps and source indices
  // (zeros when the layer carries none), intensity (empty when the observations carry none).  Throws on an unknown name.
  struct LayerDump {
    std::vector<float> x, y, z, t, intensity;
    std::vector<uint32_t> src_idx;
    bool alive = false;  // among the layers handed to ICP
  };
  LayerDump downloadLayer(const std::string& name) const;
  // A local map by name as mh_map_download gives it: points voxel by voxel, voxels in ascending (kx, ky, kz).
  struct MapDump {
    std::vector<float> x, y, z;
    std::vector<uint32_t> src_idx, vox_first, vox_count;
    std::vector<int32_t> vox_keys;  // 3 per voxel
  };
  MapDump downloadMap(const std::string& name) const;
  // A CVoxelMap local map by name as mh_occmap_download gives it: every stored cell's indices (3 per cell, ascending key
  // order) and log-odds.  (downloadMap, localMapSizes and localMapStats report such a map's occupied centres.)
  struct VoxelMapDump {
    std::vector<int32_t> keys, logodds;
    float search_voxel_size = 0.f;  // the voxel of the search map over the occupied centres (it grows with the matchers' radii)
  };
  VoxelMapDump downloadVoxelMap(const std::string& name) const;
  std::map<std::string, double> dynamicVariables() const { return source_.getVariableValues(); }
  // what initialize() recognised in the pipeline file (for tests / logs)
  std::map<std::string, std::string> describePipeline() const;
  // accumulated host wall time [s] per stage of onLidar (the role of the reference's profiler_ sections "onLidar.*")
  const std::map<std::string, double>& profile() const { return profile_; }
  void resetProfile() { profile_.clear(); }
  // The interleaved buffers handed to onLidarInterleaved / prefetchInterleaved are page-locked (mh_host_alloc_pinned) and
  // stay valid and unmodified until the scan AFTER the one they hold has been registered: uploads are then asynchronous.
  void setInputPinned(bool pinned) { input_pinned_ = pinned; }  // e.g. after the warm-up scans of a replay: steady-state stage times

 private:
  struct FilterPlan;  // the recognised observation filter chain, as data for mh_scan_preprocess / mh_scan_deskew
  struct GeneralPlan;  // any other chain of the implemented filters: ordered steps over named device layers, several maps
  struct RawInput;  // where the points of the current observation come from
  struct Prefetch;  // the announced next observation and its worker
  const ScanRecord& process(double timestamp, const RawInput& in);
  void launch_prefetch();
  void cancel_prefetch();
  void updatePipelineDynamicVariables();
  void updatePipelineTwistVariables(const Twist& tw);
  void run_first_pass();
  void run_second_pass();
  void doUpdateAdaptiveThreshold(const CPose3D& motionModelError);
  void create_local_map();
  std::shared_ptr<HashedVoxelPointCloud> make_map(const Config& def, double* voxel_size, float* remove_far) const;
  void run_general_pass(int pass);
  void run_generator(const RawInput& in);
  void merge_sensors(const std::vector<std::string>& labels, const std::vector<mh_merge_source>& srcs, DevicePointCloud& out);
  void refuse_unlabelled(const char* what) const;  // rigs take onLidarFrom only  // depth-image plans: the observations_generator step
  void record_layer_sizes(ScanRecord& rec) const;  // general plans: layer_sizes, n_for_icp, n_for_map of the live layers
  uint64_t maps_total(bool voxels) const;
  void ensure_device();
  void restore_loaded_maps();                                // load_existing_local_map: the maps from the file's records
  void seed_motion_model(double t, const CPose3D& pose);     // fuse `pose` at t - 0.2 and t - 0.1 (:779-794)
  void scan_layers(mp2p_icp_hip::metric_map_t& obs, mp2p_icp_hip::metric_map_t& glob) const;  // what this scan's ICP aligns
  void serve_relocalization(double t, ScanRecord& rec);
  std::vector<TPose3D> place_candidates(ScanRecord& rec, double step);  // steps 1-3 of relocalizeInKeyFrames
  double reloc_score_threshold(const std::string& global_layer) const;  // NaN while the searched map is not there
  void store_keyframe(ScanRecord& rec, bool first_scan, bool icp_good, const double* cov);  // params.simplemap.generate
  std::vector<molahip_host::KeyFrameTarget> keyframe_targets() const;  // the plan's maps as the key-frame file's header names them
  void check_loaded_keyframe_targets(const std::vector<molahip_host::KeyFrameTarget>& plan) const;  // throws on another class or mh_map_params
  void resolve_map_counts() const;  // fills n_map_points / n_map_voxels of the records that still wait for them
  bool map_is_empty();              // local_map_->empty() without a device round trip once the map is known to hold points
  void feed_loop_closer(ScanRecord& rec);                        // online_loop_closure: the stored frames not pushed yet; feedback
  void apply_loop_correction(ScanRecord& rec, const CPose3D& stored_pose_before);  // ... pose, motion model, local maps

  std::shared_ptr<DeviceContext> ctx_;
  Params params_;
  std::unique_ptr<FilterPlan> plan_;
  std::unique_ptr<GeneralPlan> gplan_;  // set instead of plan_ when FilterPlan does not recognise the chain
  ParameterSource source_;
  NavStateFuse navstate_;
  ICP::Ptr icp_[2];  // [0] RegularOdometry, [1] NoMotionModel
  mp2p_icp_hip::Parameters icp_params_[2];
  Config map_def_;

  // observation layers (device)
  std::shared_ptr<DevicePointCloud> raw_, map_skewed_, icp_skewed_, for_map_, for_icp_;
  // prefetch: a second context (stream + scratch) used by the worker thread only, with two sets of raw / skewed layers
  // filled alternately (the current scan may still re-de-skew from its set while the next one is being prepared)
  std::shared_ptr<DeviceContext> ctx_b_;
  float icp_bb_min_[3] = {0, 0, 0}, icp_bb_max_[3] = {0, 0, 0};  // bounding box of for_icp_ (run_second_pass)
  std::shared_ptr<mp2p_icp_hip::AlignBatcher> batcher_;  // set: filters and alignments join those of the other sequences
  std::shared_ptr<DevicePointCloud> raw_b_[2], map_skewed_b_[2], icp_skewed_b_[2];
  std::shared_ptr<DevicePointCloud> cur_raw_, cur_map_skewed_, cur_icp_skewed_;  // the set the current scan reads
  std::unique_ptr<Prefetch> pf_;
  std::shared_ptr<HashedVoxelPointCloud> local_map_;
  float remove_voxels_farther_than_ = 0.f;
  double map_voxel_size_ = 0;

  // state_ (LidarOdometry.h: struct MethodState)
  CPose3D last_lidar_pose_;
  bool last_icp_was_good_ = true;
  double last_icp_quality_ = 0;
  // rigs: the waiting set, the device layer and mounting pose of every label, the per-label times of the drop test (:647-650, 763)
  SensorSync sync_;
  struct SensorSlot {
    std::shared_ptr<DevicePointCloud> cloud;
    double pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  };
  std::map<std::string, SensorSlot> sensors_;
  std::shared_ptr<DevicePointCloud> range_probe_;  // the first observation in the vehicle frame, for the range estimate
  std::map<std::string, double> last_obs_tim_by_label_;
  std::vector<std::regex> label_patterns_;  // params_.lidar_sensor_labels, compiled once
  bool labelled_seen_ = false, merged_input_ = false;
  std::optional<double> last_obs_tim_, last_icp_timestamp_, first_ever_timestamp_, last_obs_timestamp_;
  std::optional<NavStateFuse::NavState> last_motion_model_output_;
  double adapt_thres_sigma_ = 0;
  std::optional<double> estimated_sensor_max_range_, instantaneous_sensor_max_range_;
  SearchablePoseList distance_checker_local_map_;
  uint32_t localmap_check_removal_counter_ = 0;
  std::vector<std::pair<double, CPose3D>> trajectory_;
  mutable std::vector<ScanRecord> records_;
  mutable bool map_counts_pending_ = false;  // records_[map_counts_from_ ...] wait for the map's counters
  mutable size_t map_counts_from_ = 0;
  mutable uint64_t map_points_cached_ = 0, map_voxels_cached_ = 0;
  mutable bool map_known_nonempty_ = false;
  InitialLocalization init_loc_;
  RelocalizationOptions reloc_opts_;
  std::vector<molahip_host::LocalMapRecord> loaded_maps_;  // load_existing_local_map, read at initialize()
  KeyFrameStore kf_store_;
  molahip_host::KeyFrameSet loaded_keyframes_;  // load_existing_simple_map, read at initialize()
  bool kf_targets_known_ = false;               // the header's target maps are final once the maps exist (their $f{} formulas)
  bool initial_localization_done_ = false;
  struct RelocRequest {
    CPose3D mean;
    double cov[36];
    bool in_keyframes = false;  // relocalizeInKeyFrames: mean and cov come from the place search at the serving scan
  };
  std::optional<RelocRequest> reloc_request_;
  // what relocalizeNearPose / relocalizeInKeyFrames refuse of the batcher, of `mean` (when given) and of the plan, in this order;
  // -> the layers to score with
  void check_can_relocalize(const char* who, std::string& global_layer, std::string& local_layer, const CPose3D* mean = nullptr) const;
  void note_served(ScanRecord& rec, double seconds);  // lost_recovery: a request was served, in `seconds`; rec.relocalized says how
  void place_recovery_request(uint32_t kind);        // lost_recovery: the driver's own request through the public calls
  void near_attempt_cov(double cov[36]) const;       // ... the covariance of a `near` attempt
  bool near_attempt_fits() const;                    // ... and whether its grid stays within relocalization.max_candidates
  LostRecovery lost_;                                // lost_recovery: (used only when its options are enabled)
  CPose3D lost_pose_;                                // ... the last good pose when the driver became LOST
  std::string recovery_error_;                       // ... lastRecoveryError()
  std::unique_ptr<PlaceIndex> place_index_;  // relocalizeInKeyFrames: built at the first serving scan
  size_t place_frames_seen_ = 0;             // ... and how many frames of the key-frame store it has looked at
  // online_loop_closure:
  bool loop_enabled_ = false, loop_correct_ = true;
  Config loop_cfg_;                               // the pipeline file, for the closer (made when the target maps are known)
  std::shared_ptr<OnlineLoopCloser> loop_closer_;
  size_t loop_pushed_ = 0;                        // frames of the key-frame store the closer has
  struct TrajectoryAnchor {
    long frame = -1;  // the last stored frame at or before the entry (-1: none yet)
    CPose3D rel;      // the entry's pose in that frame, when it was made
  };
  std::vector<TrajectoryAnchor> trajectory_anchor_;  // one per trajectory_ entry (kept while enabled)
  // online_map_cleaning:
  OnlineMapCleaningOptions live_opts_;
  std::unique_ptr<LiveMapCleaner> live_cleaner_;  // made at the first local map update (the maps and their context exist then)
  bool clean_live_maps();                          // the rule of LiveMapCleaner behind this scan's insertions
  // gyro_deskew:
  GyroDeskewOptions gyro_opts_;
  GyroBuffer gyro_buf_;
  std::optional<MotionTable> gyro_table_;  // the rotations of the current scan's sweep (v is set at every use)
  uint64_t scans_gyro_deskewed_ = 0;
  bool input_pinned_ = false;
  bool intensity_input_ = false;  // setIntensityInput
  std::map<std::string, double> profile_;
};

// the relocalization: block of a pipeline file as initialize() reads it (defaults when absent; std::runtime_error on values out of range)
LidarOdometry::RelocalizationOptions relocalization_options(const Config& pipeline);

}  // namespace mola_hip
