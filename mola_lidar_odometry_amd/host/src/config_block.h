// config_block.h -- one reader for the top-level option blocks of the pipeline file that this implementation adds (occupancy_grid:,
// traversability:, costmap:, gyro_deskew:, map_cleaning:, online_map_cleaning:).  Internal to host/src.  An absent or null key leaves
// the value as it is; every refusal is std::runtime_error "<block>: <key> <what>".
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "molahip_host/keyframe_file.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"

namespace mola_hip {

[[noreturn]] inline void bad_option(const std::string& block, const std::string& key, const std::string& what) {
  throw std::runtime_error(block + ": " + key + " " + what);
}

// what a block's target_map key names among the key-frame set's target maps; empty: the first.  `who` is the calling function.
inline size_t target_map_index(const molahip_host::KeyFrameSet& set, const std::string& target_map, const char* who, const char* block) {
  if (set.maps.empty()) throw std::runtime_error(std::string(who) + ": the key-frame set names no target map");
  if (target_map.empty()) return 0;
  for (size_t i = 0; i < set.maps.size(); i++)
    if (set.maps[i].name == target_map) return i;
  throw std::runtime_error(std::string(who) + ": " + block + ": target_map '" + target_map + "' is not a target map of the key-frame set");
}

class ConfigBlock {
 public:
  ConfigBlock(const mp2p_icp_hip::Config& block, std::string name) : c_(block), name_(std::move(name)) {}

  [[noreturn]] void bad(const std::string& key, const std::string& what) const { bad_option(name_, key, what); }

  // a key that is neither among `own` nor among `shared` is refused
  void knownKeys(std::initializer_list<const char*> own, const std::vector<std::string>& shared = {}) const {
    for (const auto& kv : c_.map)
      if (std::find(own.begin(), own.end(), kv.first) == own.end() && std::find(shared.begin(), shared.end(), kv.first) == shared.end())
        bad(kv.first, "is not a key of this block");
  }

  void number(const char* k, double& v) const {
    if (const auto* s = value(k)) v = toNumber(*s, k, "must be a number");
  }
  void numbers(const char* k, double* v, size_t n) const {
    const auto* s = value(k);
    if (!s) return;
    const std::string what = "must be a list of " + std::to_string(n) + " numbers";
    if (s->kind != mp2p_icp_hip::Config::Kind::Seq || s->seq.size() != n) bad(k, what);
    for (size_t i = 0; i < n; i++) v[i] = toNumber(s->at(i), k, what);
  }
  void count(const char* k, uint32_t& v) const {
    double d = v;
    number(k, d);
    if (!(d >= 0.0) || !(d <= 4294967295.0) || d != std::floor(d)) bad(k, "must be an integer >= 0");
    v = (uint32_t)d;
  }
  void boolean(const char* k, bool& v) const {
    const auto* c = value(k);
    if (!c) return;
    const std::string s = c->asString();
    if (s == "true" || s == "True" || s == "1" || s == "yes") v = true;
    else if (s == "false" || s == "False" || s == "0" || s == "no") v = false;
    else bad(k, "must be true or false");
  }
  void text(const char* k, std::string& v) const {
    if (const auto* s = value(k)) v = s->asString();
  }

  // the key's value, or nullptr when the key is absent or null
  const mp2p_icp_hip::Config* value(const char* k) const { return c_.has(k) && !c_[k].isNull() ? &c_[k] : nullptr; }

 private:
  // `not_scalar`: what is wrong with a list or a map in this place
  double toNumber(const mp2p_icp_hip::Config& s, const char* k, const std::string& not_scalar) const {
    if (s.kind != mp2p_icp_hip::Config::Kind::Scalar) bad(k, not_scalar);
    const std::string t = s.asString();
    char* end = nullptr;
    const double v = strtod(t.c_str(), &end);
    if (end == t.c_str() || *end != '\0') bad(k, "must be a number");
    return v;
  }

  const mp2p_icp_hip::Config& c_;
  std::string name_;
};

}  // namespace mola_hip
