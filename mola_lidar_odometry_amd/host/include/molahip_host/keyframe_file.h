// keyframe_file.h -- the file the key-frames of a mapping session are saved to (the role of the reference's simplemap:
// params.simplemap, --output-simplemap, LidarOdometry.cpp:1117-1138, 1209-1296).  Host arrays only, in the style of
// local_map_file.h: the format can be written, read and tested without a device.  A file holds the target maps of the plan that
// recorded it -- what a LocalMapRecord holds without its points -- and the key-frames in the order they were taken.  A key-frame
// carries the layers its FilterMerge steps would have merged (vehicle frame, de-skewed, decimated), not the raw observation:
// mola_hip::build_session_maps turns a file into the maps of the whole drive with one mh_map_insert_frames per map.
//
// Byte layout, little-endian, no padding (INTEGRATION.md has the same table):
//   char[8]  magic "MHKEYFRM"
//   u32      format version (kKeyFrameFileVersion = 1)
//   u32      number of target maps
//   per target map:
//     u32 + bytes   name        (length, then that many bytes, no terminator)
//     u32 + bytes   class       ("HashedVoxelPointCloud", "NDT", "SparseTreesPointCloud" or "CVoxelMap")
//     f32 voxel_size | u32 max_points_per_voxel | u32 index_mode | f32 min_distance_between_points |
//     f32 ndt_max_eigen_ratio | u32 ndt_min_points | u32 far_voxel_metric              (every field of mh_map_params, in order)
//     f32      remove_voxels_farther_than
//   u64      number of frames
//   per frame:
//     f64      timestamp
//     f64[12]  pose, row-major 3x4
//     f64[36]  covariance of the pose, row-major 6x6 in (x, y, z, yaw, pitch, roll); zeros for a first scan
//     u8       has_twist;  f64[6] twist (vx vy vz wx wy wz) when has_twist == 1
//     u8       has_points  (0: a frame without points, add_non_keyframes_too)
//     when has_points == 1:
//       u32      number of entries (one per FilterMerge step of insert_observation_into_local_map, in step order)
//       per entry:  u32 target map index | u64 n | f32[n] x | f32[n] y | f32[n] z
//   u64      checksum: FNV-1a (64 bit) over every byte before it
// The reader refuses -- std::runtime_error naming the file and the reason -- a wrong magic, a newer version, a truncated file,
// trailing bytes, a failed checksum, a flag byte that is neither 0 nor 1 and an entry whose map index the header does not hold.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "molahip.h"

namespace molahip_host {

constexpr uint32_t kKeyFrameFileVersion = 1;

struct KeyFrameTarget {  // a LocalMapRecord without its points
  std::string name, class_name;
  mh_map_params params{};
  float remove_voxels_farther_than = 0.f;
};

struct KeyFrameLayer {  // the input layer of one FilterMerge step
  uint32_t map_index = 0;
  std::vector<float> x, y, z;
};

struct KeyFrame {
  double timestamp = 0;
  double pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double cov[36] = {0};
  bool has_twist = false;
  double twist[6] = {0, 0, 0, 0, 0, 0};
  bool has_points = false;
  std::vector<KeyFrameLayer> layers;  // has_points only
};

struct KeyFrameSet {
  std::vector<KeyFrameTarget> maps;
  std::vector<KeyFrame> frames;
};

void write_keyframe_file(const std::string& path, const KeyFrameSet& set);
KeyFrameSet read_keyframe_file(const std::string& path);

}  // namespace molahip_host
