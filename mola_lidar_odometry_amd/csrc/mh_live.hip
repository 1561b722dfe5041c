// mh_live.hip -- erasing moving objects from a live local map: mh_views_put_scan, mh_views_vote_map, mh_map_erase_points,
// mh_map_erase_seen_through (kernels in mh_k_live.h; the specification is the text of include/molahip_live.h).
//
// put_scan:  the slot preset to "empty", one k_view_put over the scan's points.  Queued.
// vote_map:  k_vote_map over the map's records, kLiveLaunchViews neighbours per launch; NDT maps take their point records'
//            words into download order with k_live_pick.
// erase:     keep flags per stored point (k_live_keep), an exclusive scan, the kept points in order to the front of the map's
//            merge arrays (k_live_compact), then the rebuild every update of a map runs (map_build_device, every input a stored
//            point): keys, heads, k_keep, compaction, NDT statistics, slot table.  There is no second rebuild here.
// Everything is ordered on the context's stream, the one views are written on and maps are updated on.
#include <math.h>
#include <string.h>
#include <cstring>

#include <algorithm>

#include <rocprim/rocprim.hpp>

#include "molahip_live.h"
#include "mh_internal.h"
#include "mh_views.h"
#include "mh_k_live.h"

using namespace mh;

namespace {

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
inline bool mem_ok(int32_t mem) { return mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED; }

mh_status nbr_ok(const char* fn, const mh_views* v, uint32_t n_nbr, const uint32_t* nbr_view, const double* nbr_T) {
  if (n_nbr > MH_LIVE_MAX_VIEWS) return fail(MH_ERR_INVALID_ARGUMENT, "%s: more than MH_LIVE_MAX_VIEWS neighbours", fn);
  if (n_nbr && !(nbr_view && nbr_T)) return fail(MH_ERR_INVALID_ARGUMENT, "%s: null neighbour list", fn);
  for (uint32_t k = 0; k < n_nbr; k++) {
    if (nbr_view[k] >= v->size) return fail(MH_ERR_INVALID_ARGUMENT, "%s: neighbour index beyond the store", fn);
    for (int e = 0; e < 12; e++)
      if (!isfinite(nbr_T[12 * (size_t)k + e])) return fail(MH_ERR_INVALID_ARGUMENT, "%s: non-finite pose entry", fn);
  }
  return MH_OK;
}

// votes[r] for every record of the map; `votes` holds m->n_records words of device memory (the true count, or the host's bound
// of it while the last update's counts are on their way: the kernel stops at the device's own count)
mh_status vote_records(const mh_views* v, const mh_map* m, uint32_t n_nbr, const uint32_t* nbr_view, const double* nbr_T,
                       uint32_t* votes, hipStream_t s) {
  const uint32_t R = (uint32_t)m->n_records;
  if (!m->d_counters) return fail(MH_ERR_INVALID_ARGUMENT, "the map's last update failed: it has no counters to go by");
  if (n_nbr == 0) {
    MH_HIP(hipMemsetAsync(votes, 0, (size_t)R * sizeof(uint32_t), s));
    return MH_OK;
  }
  for (uint32_t k0 = 0; k0 < n_nbr; k0 += kLiveLaunchViews) {
    const uint32_t nk = std::min(n_nbr - k0, kLiveLaunchViews);
    LiveNbr nb{};
    for (uint32_t k = 0; k < nk; k++) {
      nb.view[k] = nbr_view[k0 + k];
      for (int e = 0; e < 12; e++) nb.T[k][e] = nbr_T[12 * (size_t)(k0 + k) + e];
    }
    hipLaunchKernelGGL(k_vote_map, dim3(nblk(R, kLiveBlock)), dim3(kLiveBlock), 0, s, (const float4*)m->pts.as<float4>(),
                       (const uint32_t*)m->d_counters, nb, nk, (const uint32_t*)v->img.as<uint32_t>(), v->tab, k0 ? 1u : 0u, votes);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// The erasing rebuild.  m->n_points / n_voxels / n_records are the true counts, or the host's bounds of them while the last
// update's counts are on their way (n_points > 0 either way).  The decision comes from `votes` (per record, with the two
// thresholds) or from `drop` (per stored point); both are device memory.
mh_status erase_queue(mh_map* m, const uint32_t* votes, uint32_t min_through_votes, uint32_t agree_weight, const uint8_t* drop) {
  if (!m->d_counters) return fail(MH_ERR_INVALID_ARGUMENT, "the map's last update failed: it has no counters to go by");
  const Switches sw = read_switches();
  hipStream_t s = m->ctx->stream;
  const size_t n = m->n_points, n_vox = m->n_voxels;
  const uint32_t N = (uint32_t)n, ndt = m->params.ndt_max_eigen_ratio > 0.f ? 1u : 0u;
  const size_t stride = up256(n * sizeof(float));
  MH_TRY(m->merge.reserve(4 * stride));
  MH_TRY(m->build_c.reserve(2 * n * sizeof(uint32_t)));  // keep | pos  (the rebuild's head | vid1 afterwards)
  if (!m->h_live) {
    MH_TRY(m->d_live.reserve(sizeof(LiveCarry)));
    MH_HIP(hipHostMalloc((void**)&m->h_live, sizeof(LiveCarry), hipHostMallocDefault));
    m->h_live[0] = m->h_live[1] = 0;
    MH_HIP(hipMemsetAsync(m->d_live.p, 0, sizeof(LiveCarry), s));
  }
  LiveCarry* carry = m->d_live.as<LiveCarry>();
  if (m->live_flag_taken) {  // (the host has taken the carried verdict in: it is reported once)
    MH_HIP(hipMemsetAsync(&carry->flag, 0, sizeof(carry->flag), s));
    m->live_flag_taken = false;
  }
  uint32_t* keep = m->build_c.as<uint32_t>();
  uint32_t* pos = keep + n;
  size_t tmp = 0;
  MH_HIP(rocprim::exclusive_scan(nullptr, tmp, keep, pos, 0u, N, rocprim::plus<uint32_t>(), s));
  MH_TRY(m->sort_tmp.reserve(tmp));
  char* base = m->merge.as<char>();
  float *mx = (float*)base, *my = (float*)(base + stride), *mz = (float*)(base + 2 * stride);
  uint32_t* msrc = (uint32_t*)(base + 3 * stride);
  const uint32_t* vf = m->vox_first.as<uint32_t>();
  const uint32_t* vc = m->vox_count.as<uint32_t>();
  const uint32_t* counters = m->d_counters;  // of the update this erasing follows
  // (counts already taken in: so is that update's verdict -- it is not carried a second time)
  const uint32_t carry_flag = m->counts_pending ? 1u : 0u;
  MH_HIP(hipMemsetAsync(keep, 0, n * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_live_keep, dim3(nblk(n_vox, 128)), dim3(128), 0, s, vf, vc, counters, ndt, votes, min_through_votes, agree_weight,
                     drop, keep);
  size_t tb = m->sort_tmp.bytes;
  MH_HIP(rocprim::exclusive_scan(m->sort_tmp.p, tb, keep, pos, 0u, N, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_live_compact, dim3(nblk(n, 256)), dim3(256), 0, s, (const float4*)m->pts.as<float4>(), vf, vc, counters, ndt,
                     (const uint32_t*)keep, (const uint32_t*)pos, N, carry_flag, carry, mx, my, mz, msrc);
  MH_HIP(hipGetLastError());
  // ahead of the rebuild's own read-back and of the event behind it: whoever has waited for that event finds both
  MH_HIP(hipMemcpyAsync(m->h_live, carry, sizeof(LiveCarry), hipMemcpyDeviceToHost, s));
  MH_TRY(map_build_device(sw, m, s, mx, my, mz, msrc, n, nullptr, n));  // every input is a stored point: nothing to sort or to test
  m->live_pending = true;
  return MH_OK;
}

}  // namespace

extern "C" {

uint32_t mh_live_api_version(void) { return MH_LIVE_API_VERSION; }

mh_status mh_views_put_scan(mh_views* v, uint64_t slot, const mh_scan* scan) {
  MH_REQUIRE(v && scan, "null argument");
  MH_REQUIRE(v->ctx == scan->ctx, "views and scan belong to different contexts");
  MH_REQUIRE(slot <= v->size, "slot beyond the end of the store");
  MH_REQUIRE(v->size < 0xFFFFFFF0ull && scan->n < 0x7FFFFFF0ull, "too many views or points");
  mh_ctx* ctx = v->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t AS = (size_t)v->tab.A * v->tab.S;
  if (slot == v->size) MH_TRY(views_reserve(v, v->size + 1));
  uint32_t* view = v->img.as<uint32_t>() + slot * AS;
  MH_HIP(hipMemsetAsync(view, 0xFF, AS * sizeof(uint32_t), s));  // all empty
  if (scan->n) {
    hipLaunchKernelGGL(k_view_put, dim3(nblk(scan->n, kPlaceChunk)), dim3(kPlaceBlock), 0, s, scan->x, scan->y, scan->z,
                       (uint32_t)scan->n, v->tab, view);
    MH_HIP(hipGetLastError());
  }
  if (slot == v->size) v->size++;
  return MH_OK;
}

mh_status mh_views_vote_map(const mh_views* v, const mh_map* m, uint32_t n_nbr, const uint32_t* nbr_view, const double* nbr_T,
                            uint32_t* votes_out, uint64_t capacity, int32_t mem) {
  MH_REQUIRE(v && m, "null argument");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  MH_REQUIRE(v->ctx == m->ctx, "views and map belong to different contexts");
  MH_TRY(nbr_ok(__func__, v, n_nbr, nbr_view, nbr_T));
  mh_ctx* ctx = m->ctx;
  MH_TRY(set_device(ctx));
  MH_TRY(map_resolve_counts(m));
  const size_t n = m->n_points, R = m->n_records;
  MH_REQUIRE(capacity >= n, "capacity below the stored count");
  MH_REQUIRE(votes_out || n == 0, "null votes_out");
  if (n == 0) return MH_OK;
  hipStream_t s = ctx->stream;
  const bool ndt = m->params.ndt_max_eigen_ratio > 0.f, to_device = mem == MH_MEM_DEVICE;
  // per record | (NDT, or a host destination) per point
  const size_t off_pts = up256(R * sizeof(uint32_t));
  MH_TRY(ctx->compact.reserve(off_pts + n * sizeof(uint32_t)));
  uint32_t* d_rec = (!ndt && to_device) ? votes_out : ctx->compact.as<uint32_t>();
  MH_TRY(vote_records(v, m, n_nbr, nbr_view, nbr_T, d_rec, s));
  uint32_t* d_pts = d_rec;  // (without statistics records the record order is the download order)
  if (ndt) {
    d_pts = to_device ? votes_out : (uint32_t*)(ctx->compact.as<char>() + off_pts);
    hipLaunchKernelGGL(k_live_pick, dim3(nblk(m->n_voxels, 128)), dim3(128), 0, s, (const uint32_t*)m->vox_first.as<uint32_t>(),
                       (const uint32_t*)m->vox_count.as<uint32_t>(), (const uint32_t*)m->d_counters, (const uint32_t*)d_rec, d_pts);
    MH_HIP(hipGetLastError());
  }
  if (!to_device) MH_HIP(hipMemcpyAsync(votes_out, d_pts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

mh_status mh_map_erase_points(mh_map* m, const uint8_t* drop, uint64_t n, int32_t mem) {
  MH_REQUIRE(m, "null map");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  mh_ctx* ctx = m->ctx;
  MH_TRY(set_device(ctx));
  MH_TRY(map_resolve_counts(m));  // the previous update's counts, as mh_map_insert takes them in; its verdict stays recorded
  MH_REQUIRE(n == m->n_points, "n is not the stored count");
  MH_REQUIRE(drop || n == 0, "null drop");
  if (n == 0) return MH_OK;
  const uint8_t* d_drop = drop;
  if (mem != MH_MEM_DEVICE) {
    MH_TRY(ctx->staging.reserve(n));
    MH_HIP(hipMemcpyAsync(ctx->staging.p, drop, n, hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(mh::wait_stream(ctx->stream));  // (a pageable source: the caller's array may be reused)
    d_drop = ctx->staging.as<uint8_t>();
  }
  return erase_queue(m, nullptr, 0u, 0u, d_drop);
}

mh_status mh_map_erase_seen_through(mh_map* m, const mh_views* v, uint32_t n_nbr, const uint32_t* nbr_view, const double* nbr_T,
                                    uint32_t min_through_votes, uint32_t agree_weight) {
  MH_REQUIRE(m && v, "null argument");
  MH_REQUIRE(v->ctx == m->ctx, "views and map belong to different contexts");
  MH_TRY(nbr_ok(__func__, v, n_nbr, nbr_view, nbr_T));
  mh_ctx* ctx = m->ctx;
  MH_TRY(set_device(ctx));
  // (no look at the last update's counts: while they are on their way n_points / n_records are the host's bounds of them)
  if (m->n_points == 0) return MH_OK;
  MH_TRY(ctx->compact.reserve(m->n_records * sizeof(uint32_t)));
  uint32_t* votes = ctx->compact.as<uint32_t>();
  MH_TRY(vote_records(v, m, n_nbr, nbr_view, nbr_T, votes, ctx->stream));
  return erase_queue(m, votes, min_through_votes, agree_weight, nullptr);
}

mh_status mh_map_erased_total(const mh_map* m, uint64_t* n) {
  MH_REQUIRE(m && n, "null argument");
  MH_TRY(set_device(m->ctx));
  MH_TRY(map_resolve_counts(m));
  *n = m->erased_total;
  return MH_OK;
}

}  // extern "C"
