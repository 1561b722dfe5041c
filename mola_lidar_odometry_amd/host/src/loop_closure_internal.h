// loop_closure_internal.h -- what loop_closure.cpp lends to the other units of the host layer (session_join.cpp): the pair
// verification close_loops and OnlineLoopCloser run, on a grid centre of the caller's choice.  Not installed.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "mola_lidar_odometry_hip/LoopClosure.h"

namespace mola_hip {

class PairVerifier {
 public:
  // what LoopCloserCore's constructor does and throws, named `who`: the options of loop_closure: and relocalization:, the
  // no-motion-model ICP block held to check_loop_closure_icp, the maps held to be buildable from key-frames
  PairVerifier(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, std::shared_ptr<DeviceContext> ctx, const std::string& who);
  ~PairVerifier();
  PairVerifier(const PairVerifier&) = delete;
  PairVerifier& operator=(const PairVerifier&) = delete;
  // the frames submaps are built from: poses and layers are read in place, so `frames` outlives the verifier
  void setMapFrames(const std::vector<molahip_host::KeyFrame>& frames);
  const std::vector<LoopFrame>& mapFrames() const;  // ... their poses and has_points, as the candidate rules read them
  // `observed` against the submap around map frame j (every frame with points within submap_radius of path of j), from the grid of
  // (sigma_xy, sigma_yaw_deg) around `centre`; pr's candidates, ranks, quality, iterations, Z and accepted are filled
  void verify(const molahip_host::KeyFrame& observed, size_t j, const TPose3D& centre, double sigma_xy, double sigma_yaw_deg, LoopReport::Pair& pr);
  const LoopClosureOptions& options() const;
  const LidarOdometry::RelocalizationOptions& relocalization() const;
  const mh_place_params& placeParams() const;
  const std::shared_ptr<DeviceContext>& context() const;
  LoopReport& report();  // seconds and counts of submap, score and refine gather here
  static bool usable(const molahip_host::KeyFrame& f);  // has a non-empty first layer: can be described and verified
  // the part of the constructor's checks that needs no device context: the options' ranges and the maps' classes
  static void checkWithoutDevice(const std::vector<molahip_host::KeyFrameTarget>& maps, const Config& pipeline, const std::string& who);

 private:
  std::unique_ptr<LoopCloserCore> core_;
};

}  // namespace mola_hip
