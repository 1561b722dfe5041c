// local_map_file.cpp -- writer and reader of the local-map file (molahip_host/local_map_file.h has the byte layout).
#include "molahip_host/local_map_file.h"

#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace molahip_host {

namespace {

const char kMagic[8] = {'M', 'H', 'L', 'O', 'C', 'M', 'A', 'P'};

uint64_t fnv1a(const unsigned char* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

// little-endian whatever the host is
void put_u32(std::vector<unsigned char>& b, uint32_t v) {
  for (int i = 0; i < 4; i++) b.push_back((unsigned char)(v >> (8 * i)));
}
void put_u64(std::vector<unsigned char>& b, uint64_t v) {
  for (int i = 0; i < 8; i++) b.push_back((unsigned char)(v >> (8 * i)));
}
void put_f32(std::vector<unsigned char>& b, float f) {
  uint32_t v;
  memcpy(&v, &f, 4);
  put_u32(b, v);
}
void put_str(std::vector<unsigned char>& b, const std::string& s) {
  put_u32(b, (uint32_t)s.size());
  b.insert(b.end(), s.begin(), s.end());
}

struct Reader {
  const std::string& path;
  const std::vector<unsigned char>& b;
  size_t end;  // the checksum starts here
  size_t at = 0;
  [[noreturn]] void fail(const std::string& why) const { throw std::runtime_error("local map file '" + path + "': " + why); }
  void need(size_t n, const char* what) const {
    if (n > end - at) fail(std::string("truncated (inside ") + what + ")");
  }
  uint32_t u32(const char* what) {
    need(4, what);
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) v |= (uint32_t)b[at + i] << (8 * i);
    at += 4;
    return v;
  }
  uint64_t u64(const char* what) {
    need(8, what);
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)b[at + i] << (8 * i);
    at += 8;
    return v;
  }
  float f32(const char* what) {
    const uint32_t v = u32(what);
    float f;
    memcpy(&f, &v, 4);
    return f;
  }
  std::string str(const char* what) {
    const uint32_t n = u32(what);
    need(n, what);
    std::string s((const char*)&b[at], n);
    at += n;
    return s;
  }
};

}  // namespace

bool local_map_class_known(const std::string& c) { return c == "HashedVoxelPointCloud" || c == "NDT" || c == "SparseTreesPointCloud"; }

void write_local_map_file(const std::string& path, const std::vector<LocalMapRecord>& maps) {
  std::vector<unsigned char> b(kMagic, kMagic + 8);
  put_u32(b, kLocalMapFileVersion);
  put_u32(b, (uint32_t)maps.size());
  for (const LocalMapRecord& m : maps) {
    const size_t n = m.x.size();
    if (m.y.size() != n || m.z.size() != n || m.src_idx.size() != n)
      throw std::runtime_error("local map file '" + path + "': map '" + m.name + "' has arrays of different lengths");
    if (!local_map_class_known(m.class_name))
      throw std::runtime_error("local map file '" + path + "': map '" + m.name + "' is a '" + m.class_name +
                               "', which has no snapshot (HashedVoxelPointCloud, NDT, SparseTreesPointCloud have)");
    put_str(b, m.name);
    put_str(b, m.class_name);
    put_f32(b, m.params.voxel_size);
    put_u32(b, m.params.max_points_per_voxel);
    put_u32(b, m.params.index_mode);
    put_f32(b, m.params.min_distance_between_points);
    put_f32(b, m.params.ndt_max_eigen_ratio);
    put_u32(b, m.params.ndt_min_points);
    put_u32(b, m.params.far_voxel_metric);
    put_f32(b, m.remove_voxels_farther_than);
    put_u64(b, (uint64_t)n);
    put_u64(b, m.n_offered);
    for (const std::vector<float>* a : {&m.x, &m.y, &m.z})
      for (float f : *a) put_f32(b, f);
    for (uint32_t s : m.src_idx) put_u32(b, s);
  }
  put_u64(b, fnv1a(b.data(), b.size()));
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("local map file '" + path + "': cannot open for writing");
  const size_t w = fwrite(b.data(), 1, b.size(), f);
  const int rc = fclose(f);
  if (w != b.size() || rc != 0) throw std::runtime_error("local map file '" + path + "': short write");
}

std::vector<LocalMapRecord> read_local_map_file(const std::string& path) {
  std::vector<unsigned char> b;
  {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("local map file '" + path + "': cannot open for reading");
    unsigned char chunk[1 << 16];
    size_t r;
    while ((r = fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + r);
    fclose(f);
  }
  Reader rd{path, b, b.size() >= 8 ? b.size() - 8 : 0};
  if (b.size() < 8 || memcmp(b.data(), kMagic, 8) != 0) rd.fail("wrong magic (not a local map file of this library)");
  if (b.size() < 24) rd.fail("truncated (inside the header)");
  rd.at = 8;
  const uint32_t version = rd.u32("the header");
  if (version > kLocalMapFileVersion)
    rd.fail("format version " + std::to_string(version) + " is newer than this reader's (" + std::to_string(kLocalMapFileVersion) + ")");
  if (version == 0) rd.fail("format version 0 does not exist");
  const uint32_t n_maps = rd.u32("the header");
  std::vector<LocalMapRecord> maps;
  for (uint32_t k = 0; k < n_maps; k++) {
    LocalMapRecord m;
    m.name = rd.str("a map's name");
    m.class_name = rd.str("a map's class");
    m.params.voxel_size = rd.f32("a map's parameters");
    m.params.max_points_per_voxel = rd.u32("a map's parameters");
    m.params.index_mode = rd.u32("a map's parameters");
    m.params.min_distance_between_points = rd.f32("a map's parameters");
    m.params.ndt_max_eigen_ratio = rd.f32("a map's parameters");
    m.params.ndt_min_points = rd.u32("a map's parameters");
    m.params.far_voxel_metric = rd.u32("a map's parameters");
    m.remove_voxels_farther_than = rd.f32("a map's parameters");
    const uint64_t n = rd.u64("a map's counts");
    m.n_offered = rd.u64("a map's counts");
    if (n > (rd.end - rd.at) / 16) rd.fail("truncated (inside the points of map '" + m.name + "')");
    for (std::vector<float>* a : {&m.x, &m.y, &m.z}) {
      a->resize(n);
      for (uint64_t i = 0; i < n; i++) (*a)[i] = rd.f32("a map's points");
    }
    m.src_idx.resize(n);
    for (uint64_t i = 0; i < n; i++) m.src_idx[i] = rd.u32("a map's points");
    maps.push_back(std::move(m));
  }
  if (rd.at != rd.end) rd.fail("trailing bytes: " + std::to_string(rd.end - rd.at) + " after the last map");
  uint64_t stored = 0;
  for (int i = 0; i < 8; i++) stored |= (uint64_t)b[rd.end + i] << (8 * i);
  if (stored != fnv1a(b.data(), rd.end)) rd.fail("checksum mismatch (the file is damaged)");
  for (const LocalMapRecord& m : maps)
    if (!local_map_class_known(m.class_name))
      rd.fail("map '" + m.name + "' is a '" + m.class_name + "', which this loader cannot build (HashedVoxelPointCloud, NDT, SparseTreesPointCloud)");
  return maps;
}

}  // namespace molahip_host
