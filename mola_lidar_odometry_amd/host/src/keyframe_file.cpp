// keyframe_file.cpp -- writer and reader of the key-frame file (molahip_host/keyframe_file.h has the byte layout).
#include "molahip_host/keyframe_file.h"

#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace molahip_host {

namespace {

const char kMagic[8] = {'M', 'H', 'K', 'E', 'Y', 'F', 'R', 'M'};

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
void put_f64(std::vector<unsigned char>& b, double d) {
  uint64_t v;
  memcpy(&v, &d, 8);
  put_u64(b, v);
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
  [[noreturn]] void fail(const std::string& why) const { throw std::runtime_error("key-frame file '" + path + "': " + why); }
  void need(size_t n, const char* what) const {
    if (n > end - at) fail(std::string("truncated (inside ") + what + ")");
  }
  uint8_t flag(const char* what) {
    need(1, what);
    const uint8_t v = b[at++];
    if (v > 1) fail(std::string("a flag byte of ") + what + " is neither 0 nor 1");
    return v;
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
  double f64(const char* what) {
    const uint64_t v = u64(what);
    double d;
    memcpy(&d, &v, 8);
    return d;
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

void write_keyframe_file(const std::string& path, const KeyFrameSet& set) {
  std::vector<unsigned char> b(kMagic, kMagic + 8);
  put_u32(b, kKeyFrameFileVersion);
  put_u32(b, (uint32_t)set.maps.size());
  for (const KeyFrameTarget& m : set.maps) {
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
  }
  put_u64(b, (uint64_t)set.frames.size());
  for (const KeyFrame& f : set.frames) {
    put_f64(b, f.timestamp);
    for (double v : f.pose) put_f64(b, v);
    for (double v : f.cov) put_f64(b, v);
    b.push_back(f.has_twist ? 1 : 0);
    if (f.has_twist)
      for (double v : f.twist) put_f64(b, v);
    b.push_back(f.has_points ? 1 : 0);
    if (!f.has_points) {
      if (!f.layers.empty()) throw std::runtime_error("key-frame file '" + path + "': a frame without points carries layers");
      continue;
    }
    put_u32(b, (uint32_t)f.layers.size());
    for (const KeyFrameLayer& l : f.layers) {
      const size_t n = l.x.size();
      if (l.y.size() != n || l.z.size() != n) throw std::runtime_error("key-frame file '" + path + "': a layer has arrays of different lengths");
      if (l.map_index >= set.maps.size())
        throw std::runtime_error("key-frame file '" + path + "': a layer names target map " + std::to_string(l.map_index) + ", the header holds " +
                                 std::to_string(set.maps.size()));
      put_u32(b, l.map_index);
      put_u64(b, (uint64_t)n);
      for (const std::vector<float>* a : {&l.x, &l.y, &l.z})
        for (float v : *a) put_f32(b, v);
    }
  }
  put_u64(b, fnv1a(b.data(), b.size()));
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("key-frame file '" + path + "': cannot open for writing");
  const size_t w = fwrite(b.data(), 1, b.size(), f);
  const int rc = fclose(f);
  if (w != b.size() || rc != 0) throw std::runtime_error("key-frame file '" + path + "': short write");
}

KeyFrameSet read_keyframe_file(const std::string& path) {
  std::vector<unsigned char> b;
  {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("key-frame file '" + path + "': cannot open for reading");
    unsigned char chunk[1 << 16];
    size_t r;
    while ((r = fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + r);
    fclose(f);
  }
  Reader rd{path, b, b.size() >= 8 ? b.size() - 8 : 0};
  if (b.size() < 8 || memcmp(b.data(), kMagic, 8) != 0) rd.fail("wrong magic (not a key-frame file of this library)");
  if (b.size() < 24) rd.fail("truncated (inside the header)");
  rd.at = 8;
  const uint32_t version = rd.u32("the header");
  if (version > kKeyFrameFileVersion)
    rd.fail("format version " + std::to_string(version) + " is newer than this reader's (" + std::to_string(kKeyFrameFileVersion) + ")");
  if (version == 0) rd.fail("format version 0 does not exist");
  KeyFrameSet set;
  const uint32_t n_maps = rd.u32("the header");
  for (uint32_t k = 0; k < n_maps; k++) {
    KeyFrameTarget m;
    m.name = rd.str("a target map's name");
    m.class_name = rd.str("a target map's class");
    m.params.voxel_size = rd.f32("a target map's parameters");
    m.params.max_points_per_voxel = rd.u32("a target map's parameters");
    m.params.index_mode = rd.u32("a target map's parameters");
    m.params.min_distance_between_points = rd.f32("a target map's parameters");
    m.params.ndt_max_eigen_ratio = rd.f32("a target map's parameters");
    m.params.ndt_min_points = rd.u32("a target map's parameters");
    m.params.far_voxel_metric = rd.u32("a target map's parameters");
    m.remove_voxels_farther_than = rd.f32("a target map's parameters");
    set.maps.push_back(std::move(m));
  }
  const uint64_t n_frames = rd.u64("the frame count");
  if (n_frames > (rd.end - rd.at) / (8 + 12 * 8 + 36 * 8 + 2)) rd.fail("truncated (inside the frames)");
  for (uint64_t k = 0; k < n_frames; k++) {
    KeyFrame f;
    f.timestamp = rd.f64("a frame's time stamp");
    for (double& v : f.pose) v = rd.f64("a frame's pose");
    for (double& v : f.cov) v = rd.f64("a frame's covariance");
    f.has_twist = rd.flag("a frame's twist") != 0;
    if (f.has_twist)
      for (double& v : f.twist) v = rd.f64("a frame's twist");
    f.has_points = rd.flag("a frame's points") != 0;
    if (f.has_points) {
      const uint32_t n_layers = rd.u32("a frame's layers");
      if (n_layers > (rd.end - rd.at) / 12) rd.fail("truncated (inside a frame's layers)");
      for (uint32_t j = 0; j < n_layers; j++) {
        KeyFrameLayer l;
        l.map_index = rd.u32("a layer's target");
        if (l.map_index >= n_maps)
          rd.fail("a layer names target map " + std::to_string(l.map_index) + ", the header holds " + std::to_string(n_maps));
        const uint64_t n = rd.u64("a layer's size");
        if (n > (rd.end - rd.at) / 12) rd.fail("truncated (inside a layer's points)");
        for (std::vector<float>* a : {&l.x, &l.y, &l.z}) {
          a->resize(n);
          for (uint64_t i = 0; i < n; i++) (*a)[i] = rd.f32("a layer's points");
        }
        f.layers.push_back(std::move(l));
      }
    }
    set.frames.push_back(std::move(f));
  }
  if (rd.at != rd.end) rd.fail("trailing bytes: " + std::to_string(rd.end - rd.at) + " after the last frame");
  uint64_t stored = 0;
  for (int i = 0; i < 8; i++) stored |= (uint64_t)b[rd.end + i] << (8 * i);
  if (stored != fnv1a(b.data(), rd.end)) rd.fail("checksum mismatch (the file is damaged)");
  return set;
}

}  // namespace molahip_host
