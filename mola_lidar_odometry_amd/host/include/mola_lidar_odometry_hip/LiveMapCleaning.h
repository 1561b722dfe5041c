// LiveMapCleaning.h -- moving objects erased from the local map while driving.  MapCleaning.h cleans
// the key-frames of a recorded session before its map is built; the map the odometry registers against while it drives keeps every
// trail.  Here the driver keeps a fixed ring of views -- one per recent local map update, written from the device-resident scan that
// was just inserted -- and after an update takes out of the live maps the stored points that enough of those views look straight
// through.  Everything runs on the device through include/molahip_live.h: nothing is read back on the driving thread.
//
// THE RULE.  Views and votes are include/molahip_clean.h's, word for word; erasing is include/molahip_live.h's.  On local map
// update number u (u = 0, 1, ...; whatever clears the maps starts again at 0), after all of that update's insertPointCloud calls:
//   1. the view of view_layer's device cloud (vehicle frame) goes into slot u % max_views; the update's pose is recorded with it;
//   2. if (u + 1) % every_n_updates == 0: the neighbour list is the kept slots whose recorded position lies within
//      max_view_distance of this update's pose -- ((dx*dx + dy*dy) + dz*dz) <= max_view_distance^2, closed, fp64, as
//      cleaning_neighbours compares -- in ascending slot order, this update's own slot included; nbr_T of a slot is
//      cleaning_relative_pose(identity, recorded pose): the world-to-view transform; one mh_map_erase_seen_through(min_through_votes,
//      agree_weight) runs per target map.
// Key-frames go into the key-frame store as recorded: MapCleaning.h still applies to the file afterwards.  With the block enabled
// the session map of the merged key-frames is no longer the local map.
//
// Not built: votes carried across updates (every erasing votes afresh against the ring); a source-index gate that votes only on
// recently inserted points; the vote folded into the insertion's own rebuild (an erasing is a second rebuild); rigs with several
// sensor origins (one origin per block: a merged multi-LiDAR cloud is binned as if seen from it).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "molahip_live.h"
#include "mola_lidar_odometry_hip/MapCleaning.h"

namespace mola_hip {

using mp2p_icp_hip::CPose3D;
using mp2p_icp_hip::DevicePointCloud;
using mp2p_icp_hip::HashedVoxelPointCloud;

// the optional top-level online_map_cleaning: block of the pipeline file (this implementation's own key).  Absent, or enabled:
// false: off.  The keys of the view and the vote (n_rings .. win_sectors, max_view_distance, min_through_votes, agree_weight) have
// the names, defaults and ranges of map_cleaning: (the inherited fields; max_views_per_frame is not a key here).  An unknown key,
// or a value outside its range: std::runtime_error naming online_map_cleaning: and the key -- read and checked whether enabled or not.
struct OnlineMapCleaningOptions : MapCleaningOptions {
  bool enabled = false;
  uint32_t max_views = 24;         // slots of the ring, 1 .. MH_LIVE_MAX_VIEWS
  uint32_t every_n_updates = 1;    // >= 1
  std::string view_layer;          // "": the source layer of the plan's first FilterMerge
  std::vector<std::string> target_maps;  // empty: every point map of the plan
  static OnlineMapCleaningOptions FromConfig(const Config& pipeline);
  void validate() const;
};

// ---- host rules (testable without a device)
// step 2: slot_poses holds 12 doubles per kept slot (slots 0 .. n-1); the slots within max_view_distance of `pose`, ascending
std::vector<uint32_t> live_ring_neighbours(const std::vector<double>& slot_poses, const double pose[12], double max_view_distance);
// the host half of the ring: which slot an update writes, the poses recorded with the kept slots, whether an erasing is due
class LiveRing {
 public:
  LiveRing(uint32_t max_views, uint32_t every_n_updates) : max_views_(max_views), every_(every_n_updates) {}
  struct Step {
    uint32_t slot = 0;  // updates() % max_views before the call
    bool due = false;   // (updates() + 1) % every_n_updates == 0
  };
  Step put(const double pose[12]);  // local map update number updates(): step 1's bookkeeping
  std::vector<uint32_t> neighbours(const double pose[12], double max_view_distance) const {
    return live_ring_neighbours(slot_poses_, pose, max_view_distance);
  }
  const double* pose(uint32_t slot) const { return &slot_poses_[12 * (size_t)slot]; }
  void clear() { slot_poses_.clear(); u_ = 0; }  // (the next update is number 0; the view store keeps its slots: they are written before they are read)
  uint64_t updates() const { return u_; }
  size_t kept() const { return slot_poses_.size() / 12; }

 private:
  uint32_t max_views_, every_;
  std::vector<double> slot_poses_;  // 12 per kept slot
  uint64_t u_ = 0;
};

// The ring of views and their poses, and the rule above.  One per driver; the views live on the context of the maps.
class LiveMapCleaner {
 public:
  LiveMapCleaner(const OnlineMapCleaningOptions& opt, std::shared_ptr<DeviceContext> ctx);
  ~LiveMapCleaner();
  LiveMapCleaner(const LiveMapCleaner&) = delete;
  // the next local map update: steps 1 and 2.  `view` is the cloud of view_layer, `pose` the update's pose, `targets` the maps to
  // erase from.  Returns whether the maps were voted on (step 2 was due).  Queued: no host wait.
  bool update(const DevicePointCloud& view, const CPose3D& pose, const std::vector<HashedVoxelPointCloud*>& targets);
  void clear() { ring_.clear(); }  // whatever clears the maps: the ring is empty
  const LiveRing& ring() const { return ring_; }
  const OnlineMapCleaningOptions& options() const { return opt_; }

 private:
  OnlineMapCleaningOptions opt_;
  std::shared_ptr<DeviceContext> ctx_;
  mh_views* views_ = nullptr;
  LiveRing ring_;
};

}  // namespace mola_hip
