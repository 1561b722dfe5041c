// local_map_file.h -- the file a device local map is saved to and restored from (HashedVoxelPointCloud::saveToFile /
// loadFromFile, LidarOdometry::saveLocalMaps, params.local_map_updates.load_existing_local_map).  Host arrays only: the
// format can be written, read and tested without a device.  One file holds several NAMED maps (a general plan has one per
// localmap_generator entry).  Per map: what mh_map_download returns (points voxel by voxel, voxels in ascending packed key,
// in-voxel insertion order, the source index of every point) plus mh_map_info::n_offered -- the input of mh_map_restore -- with
// the parameters the map was created with.
//
// Byte layout, little-endian, no padding (INTEGRATION.md has the same table):
//   char[8]  magic "MHLOCMAP"
//   u32      format version (kLocalMapFileVersion = 1)
//   u32      number of maps
//   per map:
//     u32 + bytes   name        (length, then that many bytes, no terminator)
//     u32 + bytes   class       ("HashedVoxelPointCloud", "NDT" or "SparseTreesPointCloud")
//     f32 voxel_size | u32 max_points_per_voxel | u32 index_mode | f32 min_distance_between_points |
//     f32 ndt_max_eigen_ratio | u32 ndt_min_points | u32 far_voxel_metric              (every field of mh_map_params, in order)
//     f32      remove_voxels_farther_than  (the insertion option the driver keeps beside the map)
//     u64      n_points
//     u64      n_offered
//     f32[n_points] x | f32[n_points] y | f32[n_points] z | u32[n_points] src_idx
//   u64      checksum: FNV-1a (64 bit) over every byte before it
// The reader refuses -- std::runtime_error naming the file and the reason -- a wrong magic, a newer version, a truncated file,
// trailing bytes, a failed checksum, and a map whose class the loader cannot build.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "molahip.h"

namespace molahip_host {

constexpr uint32_t kLocalMapFileVersion = 1;

struct LocalMapRecord {
  std::string name;        // the map's layer name (localmap_generator's layer)
  std::string class_name;  // "HashedVoxelPointCloud" | "NDT" | "SparseTreesPointCloud"
  mh_map_params params{};
  float remove_voxels_farther_than = 0.f;
  uint64_t n_offered = 0;
  std::vector<float> x, y, z;
  std::vector<uint32_t> src_idx;
};

// classes mp2p_icp_hip::make_local_map can build
bool local_map_class_known(const std::string& class_name);
void write_local_map_file(const std::string& path, const std::vector<LocalMapRecord>& maps);
std::vector<LocalMapRecord> read_local_map_file(const std::string& path);

}  // namespace molahip_host
