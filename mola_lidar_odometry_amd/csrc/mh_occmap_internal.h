// mh_occmap_internal.h -- the body of the occupancy map handle and the host helpers that mh_occmap.hip and mh_occgrid.hip share.
#pragma once
#include <string.h>  // (rocPRIM's texture iterator calls the host memset without declaring it)
#include <rocprim/rocprim.hpp>

#include "mh_k_occ.h"

struct mh_occmap {
  mh_ctx* ctx = nullptr;
  mh_occmap_params params{};
  float inv_res = 1.f;
  mh::occ::Rule rule{};
  uint64_t max_keys_per_pass = 0;
  // the store: ping-pong pair of (keys, log-odds); `cur` is the valid one
  mh::DevBuf skey[2], slo[2];
  int cur = 0;
  uint64_t n_cells = 0, n_occupied = 0;
  // the occupied centres (ascending key order) and the search map built from them
  mh::DevBuf cx, cy, cz;
  mh_map* inner = nullptr;
  float V = 1.f;
  // last insert
  uint64_t n_left_out = 0, n_keys = 0;
  uint32_t n_passes = 0;
  // scratch
  mh::DevBuf ray_e, items, prefix, counters;   // per ray
  mh::DevBuf pk, pks, rk, rc;                  // per pass: keys, sorted keys, run keys, run counts
  mh::DevBuf ak[2], ac[2], mk, mc;             // accumulated (key, count) entries of all passes; merge scratch
  mh::DevBuf head, pos, ucell, uh, um, ulb, is_new, new_rank;  // per touched cell
  mh::DevBuf mkey, mlo, flags, fscan;          // merged sequence
  mh::DevBuf tmp;                              // rocPRIM temporary storage
  // mh_occmap_insert_frames / mh_occmap_project_grid (mh_occgrid.hip)
  mh::DevBuf f_up, f_rayf, f_pf, f_pfs, f_ek, f_ev, f_ak[2], f_af[2], f_ac[2], f_ustart, f_unew, f_grid;
  mh::PinnedBuf f_h;                           // page-locked mirror of one pass's upload
  unsigned long long* h_rb = nullptr;      // pinned [4]: read-backs
};

namespace mh {
namespace occ {

constexpr uint64_t kDefaultKeysPerPass = 1ull << 24;  // 128 MiB of keys, and as much again sorted

inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

struct ToU64 {
  __host__ __device__ unsigned long long operator()(uint32_t v) const { return v; }
};

inline mh_status inner_rebuild(mh_occmap* o) {
  return mh_map_build(o->inner, o->cx.as<float>(), o->cy.as<float>(), o->cz.as<float>(), o->n_occupied, MH_MEM_DEVICE);
}

// A search map of voxel size v over the present centres in place of the present one.  The new map is complete before the old
// one goes: a failure leaves the occupancy map, its search map and its V as they were.
inline mh_status inner_replace(mh_occmap* o, float v) {
  mh_map_params mp{};
  mp.voxel_size = v;
  mp.max_points_per_voxel = 0;
  mp.index_mode = o->params.index_mode;
  mp.far_voxel_metric = o->params.far_voxel_metric;
  mh_map* fresh = nullptr;
  MH_TRY(mh_map_create(o->ctx, &mp, &fresh));
  const mh_status st = mh_map_build(fresh, o->cx.as<float>(), o->cy.as<float>(), o->cz.as<float>(), o->n_occupied, MH_MEM_DEVICE);
  if (st != MH_OK) {
    (void)mh_map_destroy(fresh);
    return st;
  }
  (void)mh_map_destroy(o->inner);
  o->inner = fresh;
  o->V = v;
  return MH_OK;
}

// read `n` 64-bit words from the device (blocking)
inline mh_status read_back(mh_occmap* o, const void* src, size_t n, hipStream_t s) {
  MH_HIP(hipMemcpyAsync(o->h_rb, src, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

template <class F>
mh_status with_tmp(mh_occmap* o, F&& call) {  // rocPRIM's two-call protocol
  size_t bytes = 0;
  MH_HIP(call(nullptr, bytes));
  MH_TRY(o->tmp.reserve(bytes ? bytes : 256));
  bytes = o->tmp.bytes;
  MH_HIP(call(o->tmp.p, bytes));
  return MH_OK;
}

}  // namespace occ
}  // namespace mh
