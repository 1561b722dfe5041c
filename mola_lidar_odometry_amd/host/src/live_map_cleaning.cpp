// live_map_cleaning.cpp -- see mola_lidar_odometry_hip/LiveMapCleaning.h.  Host logic only: the device is reached through the calls
// of include/molahip_live.h.
#include "mola_lidar_odometry_hip/LiveMapCleaning.h"

#include <algorithm>
#include <stdexcept>

#include "config_block.h"

namespace mola_hip {

using namespace mp2p_icp_hip;

namespace {
const char* const kBlock = "online_map_cleaning";
[[noreturn]] void bad(const std::string& key, const std::string& what) { bad_option(kBlock, key, what); }
}  // namespace

// ================================================================== options
OnlineMapCleaningOptions OnlineMapCleaningOptions::FromConfig(const Config& cfg) {
  OnlineMapCleaningOptions o;
  if (cfg.has(kBlock) && !cfg[kBlock].isNull()) {
    const ConfigBlock c(cfg[kBlock], kBlock);
    c.knownKeys({"enabled", "max_views", "every_n_updates", "view_layer", "target_maps"}, cleaning_shared_keys());
    c.boolean("enabled", o.enabled);
    read_cleaning_shared_keys(cfg[kBlock], kBlock, o);
    c.count("max_views", o.max_views);
    c.count("every_n_updates", o.every_n_updates);
    if (c.value("view_layer") && c.value("view_layer")->kind != Config::Kind::Scalar) bad("view_layer", "must be a layer name");
    c.text("view_layer", o.view_layer);
    if (const Config* t = c.value("target_maps")) {
      if (t->kind != Config::Kind::Seq) bad("target_maps", "must be a list of map names");
      for (size_t i = 0; i < t->size(); i++) {
        if (t->at(i).kind != Config::Kind::Scalar || t->at(i).asString().empty()) bad("target_maps", "must be a list of map names");
        if (std::find(o.target_maps.begin(), o.target_maps.end(), t->at(i).asString()) != o.target_maps.end())
          bad("target_maps", "names '" + t->at(i).asString() + "' twice");
        o.target_maps.push_back(t->at(i).asString());
      }
    }
  }
  o.validate();
  return o;
}

void OnlineMapCleaningOptions::validate() const {
  validateAs(kBlock);
  if (max_views < 1 || max_views > MH_LIVE_MAX_VIEWS) bad("max_views", "must be in 1.." + std::to_string(MH_LIVE_MAX_VIEWS));
  if (every_n_updates < 1) bad("every_n_updates", "must be an integer >= 1");
}

// ================================================================== host rules
std::vector<uint32_t> live_ring_neighbours(const std::vector<double>& slot_poses, const double pose[12], double max_view_distance) {
  if (slot_poses.size() % 12) throw std::runtime_error("live_ring_neighbours: slot_poses needs 12 values per slot");
  const double lim = max_view_distance * max_view_distance;
  std::vector<uint32_t> out;
  for (size_t s = 0; s < slot_poses.size() / 12; s++) {
    const double* b = &slot_poses[12 * s];
    const double dx = b[3] - pose[3], dy = b[7] - pose[7], dz = b[11] - pose[11];
    if ((dx * dx + dy * dy) + dz * dz <= lim) out.push_back((uint32_t)s);
  }
  return out;
}

// ================================================================== the ring
LiveRing::Step LiveRing::put(const double pose[12]) {
  Step st;
  st.slot = (uint32_t)(u_ % max_views_);
  if ((size_t)st.slot * 12 == slot_poses_.size()) slot_poses_.resize(slot_poses_.size() + 12);  // (slots fill in order, then wrap)
  std::copy(pose, pose + 12, &slot_poses_[12 * (size_t)st.slot]);
  st.due = (u_ + 1) % every_ == 0;
  u_++;
  return st;
}

LiveMapCleaner::LiveMapCleaner(const OnlineMapCleaningOptions& opt, std::shared_ptr<DeviceContext> ctx)
    : opt_(opt), ctx_(std::move(ctx)), ring_(opt.max_views, opt.every_n_updates) {
  opt_.validate();
  if (!ctx_) ctx_ = DeviceContext::Default();
  const mh_clean_params params = opt_.deviceParams();
  check(mh_views_create(ctx_->get(), &params, &views_), "mh_views_create");
}

LiveMapCleaner::~LiveMapCleaner() { mh_views_destroy(views_); }

bool LiveMapCleaner::update(const DevicePointCloud& view, const CPose3D& pose, const std::vector<HashedVoxelPointCloud*>& targets) {
  const uint32_t slot = (uint32_t)(ring_.updates() % opt_.max_views);
  check(mh_views_put_scan(views_, slot, view.handle()), "mh_views_put_scan");  // (refused: the ring is as it was)
  if (!ring_.put(pose.T).due) return false;
  const std::vector<uint32_t> nbr = ring_.neighbours(pose.T, opt_.max_view_distance);
  static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<double> nbr_T(12 * nbr.size());
  for (size_t k = 0; k < nbr.size(); k++) cleaning_relative_pose(identity, ring_.pose(nbr[k]), &nbr_T[12 * k]);
  for (HashedVoxelPointCloud* m : targets)
    check(mh_map_erase_seen_through(m->handle(), views_, (uint32_t)nbr.size(), nbr.data(), nbr_T.data(), opt_.min_through_votes,
                                    opt_.agree_weight),
          "mh_map_erase_seen_through");
  return true;
}

}  // namespace mola_hip
