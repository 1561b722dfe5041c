// MapCleaning.h -- moving objects taken out of a session's key-frames before the map is built.  The
// step between "close the loops" (LoopClosure.h) / "join the sessions" (SessionJoin.h) and build_session_maps(): drifted poses make
// distant views vote wrongly, so clean AFTER the poses are settled and BEFORE the map is built.
//
//   once   [host]    cleaning_neighbours(): which other frames look at each frame's surroundings
//   once   [device]  the views of all frames with points (ONE mh_views_add_frames; a frame's view comes from all its entries together)
//   once   [device]  the votes of every point against its frame's neighbours (ONE mh_views_vote_frames)
//   once   [host]    the decision per point, the removal per entry
//
// THE RULE.  Views and votes are include/molahip_clean.h's, word for word.  What the host adds:
//   1. Neighbours.  Frame i (with points) votes against the frames j != i with points whose positions lie within max_view_distance
//      (squared distance ((dx*dx + dy*dy) + dz*dz) <= max_view_distance^2, closed, fp64).  The nearest max_views_per_frame of them are
//      kept, ties to the lower index; the list is in ascending index order.
//   2. Relative pose.  T = T_j^-1 T_i by the entry-by-entry formula of molahip_clean.h, fp64, un-fused.
//   3. Decision.  A point is removed if and only if  through >= min_through_votes && through > agree_weight * agree  (integers).
//   4. Output.  Poses, covariances, twists, timestamps, target maps, frame count and entry order come back bit for bit; only the x, y,
//      z arrays shrink (kept points in their order).  A version-1 key-frame file: build_session_maps(), close_loops() and
//      join_sessions() take it as it is.
//
// Cleaning the live local map while driving is LiveMapCleaning.h (row g11).  Not built: per-point sensor origins for rigs (one origin per set: points of a
// merged multi-LiDAR frame are binned as if seen from it); CVoxelMap plans (refused by name, as close_loops and join_sessions do).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "molahip_clean.h"
#include "molahip_host/keyframe_file.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

using mp2p_icp_hip::Config;
using mp2p_icp_hip::DeviceContext;

// the optional top-level map_cleaning: block of the pipeline file (this implementation's own key); an absent block gives the
// defaults.  An unknown key, or a value outside its range: std::runtime_error naming map_cleaning: and the key.
struct MapCleaningOptions {
  uint32_t n_rings = 32, n_sectors = 128;      // n_sectors a multiple of 8; n_rings * n_sectors <= 4096
  double el_min_deg = -25.0, el_max_deg = 15.0;  // elevation window [deg], inside (-90, 90)
  double min_range = 2.0, max_range = 60.0;    // [m]
  double rel_margin = 0.10;                    // "farther" is beyond (1 + rel_margin) times the range
  double origin[3] = {0, 0, 0};                // the sensor's position in the vehicle frame: origin_x, origin_y, origin_z
  uint32_t win_rings = 0, win_sectors = 1;     // window half-widths, 0..2 (profiles/map_cleaning.md: why no ring window by default)
  double max_view_distance = 30.0;             // [m]
  uint32_t max_views_per_frame = 24;           // >= 1
  uint32_t min_through_votes = 2;              // >= 1
  uint32_t agree_weight = 1;                   // >= 0
  static MapCleaningOptions FromConfig(const Config& pipeline);
  void validate() const;
  void validateAs(const std::string& block) const;  // the same checks, the refusals naming another block (LiveMapCleaning.h)
  mh_clean_params deviceParams() const;  // degrees to radians in fp64, then one rounding to the struct's floats
};

// ---- what map_cleaning: and online_map_cleaning: (LiveMapCleaning.h) read alike.  `c` is the block, `block` its name in refusals.
// The keys both hold: n_rings .. win_sectors, max_view_distance, min_through_votes, agree_weight.  An absent or null key leaves its
// option as it is; anything but a number / an integer >= 0 is refused.
const std::vector<std::string>& cleaning_shared_keys();
void read_cleaning_shared_keys(const Config& c, const std::string& block, MapCleaningOptions& o);

// ---- host rules (testable without a device)
// poses: 12 doubles per frame; has_points: one flag per frame.  out[i]: the neighbours of frame i (rule 1).
std::vector<std::vector<uint32_t>> cleaning_neighbours(const std::vector<double>& poses, const std::vector<uint8_t>& has_points,
                                                       const MapCleaningOptions& opt);
// rule 2
void cleaning_relative_pose(const double Ti[12], const double Tj[12], double T[12]);
// rule 3 on a packed word of mh_views_vote_frames
inline bool cleaning_removes(uint32_t votes, const MapCleaningOptions& opt) {
  const uint64_t through = votes & 0xFFFFu, agree = votes >> 16;
  return through >= opt.min_through_votes && through > (uint64_t)opt.agree_weight * agree;
}
// rule 4 for one frame: `votes` holds one word per point over the frame's entries in order; returns the points removed
size_t cleaning_apply(molahip_host::KeyFrame& frame, const uint32_t* votes, const MapCleaningOptions& opt);

// ---- the whole thing
struct CleaningReport {
  struct Frame {
    uint64_t points_in = 0, points_removed = 0;
    uint32_t neighbours = 0;
  };
  std::vector<Frame> frames;
  uint64_t points_in = 0, points_removed = 0, pairs = 0;  // totals; pairs: (frame, neighbour) votes
  std::map<std::string, double> seconds;                   // wall time per stage: views, votes, removal
  std::string toJson() const;                              // the totals and the seconds
};
struct CleaningResult {
  molahip_host::KeyFrameSet cleaned;
  CleaningReport report;
};
// A set whose target maps include a CVoxelMap is refused by name (std::runtime_error) before any device is asked for; a set
// without any frame that has points is returned unchanged, and no device is asked for either.
CleaningResult clean_keyframes(const molahip_host::KeyFrameSet& set, const MapCleaningOptions& opt, std::shared_ptr<DeviceContext> ctx = nullptr);
// ... file to file
CleaningReport clean_keyframes_file(const std::string& input_keyframe_file, const std::string& output_keyframe_file, const MapCleaningOptions& opt,
                                    std::shared_ptr<DeviceContext> ctx = nullptr);

}  // namespace mola_hip
