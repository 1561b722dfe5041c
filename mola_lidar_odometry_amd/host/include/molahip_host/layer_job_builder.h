// layer_job_builder.h -- one multi-layer alignment as the library takes it (mh_layer_job_planes), collected pair by pair.
// Header-only and written against the C ABI alone: the mirror classes (host/src/icp.cpp) and the mp2p_icp adapter
// (host/adapters/mp2p_icp_plugin.cpp) describe their alignments through it, and AlignBatcher::alignLayers takes what it hands out.
#pragma once
#include <vector>

#include "molahip.h"

namespace molahip_host {

class LayerJobBuilder {
 public:
  /** One pair with its options: unique_global (U13), the matcher's iteration gates, its pairingsPerPoint (>= 1) and, for a
   *  Matcher_Point2Plane pair, its plane parameters (knn 0: a point pair). */
  void push(const mh_layer_pair& pair, bool unique_global, mh_layer_pair_gates gates, uint32_t pairings_per_point,
            const mh_layer_pair_plane& plane) {
    pairs_.push_back(pair);
    opts_.push_back(mh_layer_pair_opts{unique_global ? 1u : 0u});
    gates_.push_back(gates);
    knn_.push_back(mh_layer_pair_knn{pairings_per_point});
    planes_.push_back(plane);
    has_unique_ = has_unique_ || unique_global;
    has_gate_ = has_gate_ || gates.run_from_iteration || gates.run_up_to_iteration;
    has_knn_ = has_knn_ || pairings_per_point > 1;
    has_plane_ = has_plane_ || plane.knn != 0;
  }
  size_t size() const { return pairs_.size(); }
  mh_layer_pair& pair(size_t i) { return pairs_[i]; }  // (its scan and its schedule may be set after the push)
  uint32_t pairings_per_point(size_t i) const { return knn_[i].pairings_per_point; }
  bool is_plane(size_t i) const { return planes_[i].knn != 0; }
  // what the routes and the MOLA_HIP_BATCH_* switches decide on: whether any pair set that option
  bool has_unique() const { return has_unique_; }
  bool has_gate() const { return has_gate_; }
  bool has_knn() const { return has_knn_; }
  bool has_plane() const { return has_plane_; }
  /** The description; an option no pair set is a NULL array.  It points into the builder: valid until the next push. */
  mh_layer_job_planes job() const {
    return mh_layer_job_planes{pairs_.size(),
                               pairs_.data(),
                               has_unique_ ? opts_.data() : nullptr,
                               has_gate_ ? gates_.data() : nullptr,
                               has_knn_ ? knn_.data() : nullptr,
                               has_plane_ ? planes_.data() : nullptr};
  }

 private:
  std::vector<mh_layer_pair> pairs_;
  std::vector<mh_layer_pair_opts> opts_;
  std::vector<mh_layer_pair_gates> gates_;
  std::vector<mh_layer_pair_knn> knn_;
  std::vector<mh_layer_pair_plane> planes_;
  bool has_unique_ = false, has_gate_ = false, has_knn_ = false, has_plane_ = false;
};

}  // namespace molahip_host
