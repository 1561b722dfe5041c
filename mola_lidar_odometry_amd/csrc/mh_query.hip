// mh_query.hip -- map queries with a variable number of results per point: mh_nn_search_radius, the stand-in for
// mrpt::maps::NearestNeighborsCapable::nn_radius_search [U] on the hashed voxel map.  A translation unit of its own: the
// matcher, map and filter objects are built from sources this query does not touch.  Also mh_score_poses (at the end): one
// scan scored under many candidate poses in one launch (mh_k_score.h).
//
// count (k_radius<false>) -> sum / max + rocPRIM exclusive scan -> one read-back of {sum, max} -> fill (k_radius<true>)
// [-> rocPRIM stable radix sort of (query, d2 bits) -> gather] -> copies.  Scratch is the context's grow-only buffers (build_a..e,
// compact, sort_tmp): everything that uses them is ordered on the context's stream and this call blocks until it is done.
#include <math.h>
#include <string.h>  // (rocPRIM's texture iterator calls the host memset without declaring it)
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "mh_k_radius.h"
#include "mh_k_score.h"

using namespace mh;

namespace {

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

bool pose_finite(const double T[12]) {
  for (int i = 0; i < 12; i++)
    if (!isfinite(T[i])) return false;
  return true;
}

}  // namespace

extern "C" {

mh_status mh_nn_search_radius(const mh_map* map, const mh_scan* scan, const double T[12], double radius, uint32_t flags,
                              const mh_radius_out* out, int32_t mem, mh_radius_info* info) {
  // ---- refusals: all decided before anything is queued
  MH_REQUIRE(map && scan && T && info, "null argument");
  MH_REQUIRE(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE, "bad mem space");
  MH_REQUIRE(map->ctx->device == scan->ctx->device, "map and scan live on different devices");
  MH_REQUIRE(pose_finite(T), "non-finite pose");
  MH_REQUIRE(isfinite(radius) && radius > 0.0, "radius must be finite and > 0");
  MH_REQUIRE((flags & ~(uint32_t)MH_RADIUS_SORTED) == 0u, "unknown flag bits");
  const double vs = (double)map->params.voxel_size;
  if (radius > (double)MH_RADIUS_MAX_VOXELS * vs)
    return fail(MH_ERR_UNSUPPORTED, "mh_nn_search_radius: radius %g exceeds MH_RADIUS_MAX_VOXELS (%d) x voxel_size %g", radius,
                MH_RADIUS_MAX_VOXELS, vs);
  MH_REQUIRE(scan->n < 0xFFFFFFFFull, "scan size does not fit 32 bits");
  const Switches sw = read_switches();
  const mh_radius_out none{};
  if (!out) out = &none;
  const bool sorted = (flags & MH_RADIUS_SORTED) != 0u;
  info->n_results = info->n_written = 0;
  info->max_per_query = info->reserved_ = 0;

  mh_ctx* ctx = scan->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t n = scan->n;
  const hipMemcpyKind down = mem == MH_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (n == 0) {
    const uint32_t zero = 0;
    if (out->offsets) MH_HIP(hipMemcpy(out->offsets, &zero, 4, mem == MH_MEM_HOST ? hipMemcpyHostToHost : hipMemcpyHostToDevice));
    return MH_OK;
  }
  MH_TRY(map_ready_on(map, s));

  const float r2 = (float)(radius * radius);              // the square taken in fp64, rounded once
  const float rr = (float)radius * 1.00001f;               // what bounds the visited block (radius_axis)
  RadiusPose Ta;
  for (int i = 0; i < 12; i++) Ta.m[i] = T[i];
  const MapView mv = map->view(sw);

  // build_a: {sum (64 bits), max, pad} | counts[n + 1] | offsets[n + 1]
  const size_t cb = up256((n + 1) * 4);
  MH_TRY(ctx->build_a.reserve(256 + 2 * cb));
  char* a = ctx->build_a.as<char>();
  unsigned long long* d_sum = (unsigned long long*)a;
  uint32_t* d_max = (uint32_t*)(a + 8);
  uint32_t* counts = (uint32_t*)(a + 256);
  uint32_t* offsets = (uint32_t*)(a + 256 + cb);
  size_t tmp = 0;
  MH_HIP(rocprim::exclusive_scan(nullptr, tmp, counts, offsets, 0u, n + 1, rocprim::plus<uint32_t>(), s));
  MH_TRY(ctx->sort_tmp.reserve(tmp));

  // one wave per query at a time; enough waves to fill the device, each taking every n_waves-th query
  const uint32_t blocks = std::min<uint32_t>(nblk(n, kRadiusBlock / 64u), 8192u);
  MH_HIP(hipMemsetAsync(a, 0, 256, s));
  MH_HIP(hipMemsetAsync(counts + n, 0, 4, s));
  const RadiusOut no_out{};
  hipLaunchKernelGGL(k_radius<false>, dim3(blocks), dim3(kRadiusBlock), 0, s, Ta, r2, rr, scan->x, scan->y, scan->z, (uint32_t)n, mv,
                     counts, (const uint32_t*)nullptr, no_out);
  MH_HIP(hipGetLastError());
  // (few blocks: every wave ends in two atomics on the same two words, and 1 900 of them took 45 us on a 120 k-point scan)
  hipLaunchKernelGGL(k_radius_stats, dim3(std::min<uint32_t>(nblk(n, kRadiusBlock), 64u)), dim3(kRadiusBlock), 0, s, counts,
                     (uint32_t)n, d_sum, d_max);
  MH_HIP(hipGetLastError());
  size_t tb = ctx->sort_tmp.bytes;
  MH_HIP(rocprim::exclusive_scan(ctx->sort_tmp.p, tb, counts, offsets, 0u, n + 1, rocprim::plus<uint32_t>(), s));
  unsigned long long h_stats[2] = {0, 0};
  MH_HIP(hipMemcpyAsync(h_stats, a, 16, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  const uint64_t nr = h_stats[0];
  info->n_results = nr;
  info->max_per_query = (uint32_t)(h_stats[1] & 0xFFFFFFFFull);
  if (nr >= (1ull << 32)) return fail(MH_ERR_UNSUPPORTED, "mh_nn_search_radius: %llu results do not fit 32-bit offsets", (unsigned long long)nr);
  if (out->offsets) {
    MH_HIP(hipMemcpyAsync(out->offsets, offsets, (n + 1) * 4, down, s));
    MH_HIP(mh::wait_stream(s));
  }

  const bool any = out->global_idx || out->gx || out->gy || out->gz || out->d2;
  if (out->capacity < nr) return MH_OK;  // count-only call: the result arrays stay untouched
  info->n_written = nr;
  if (nr == 0 || !any) return MH_OK;

  // ---- fill.  `dst`: where the results end up on the device (the caller's arrays, or a staging block for host arrays)
  const size_t rb = up256(nr * 4);
  RadiusOut dst{};
  if (mem == MH_MEM_HOST) {
    MH_TRY(ctx->compact.reserve(5 * rb));
    char* st = ctx->compact.as<char>();
    dst.gi = out->global_idx ? (uint32_t*)st : nullptr;
    dst.x = out->gx ? (float*)(st + rb) : nullptr;
    dst.y = out->gy ? (float*)(st + 2 * rb) : nullptr;
    dst.z = out->gz ? (float*)(st + 3 * rb) : nullptr;
    dst.d2 = out->d2 ? (float*)(st + 4 * rb) : nullptr;
  } else {
    dst.gi = out->global_idx;
    dst.x = out->gx;
    dst.y = out->gy;
    dst.z = out->gz;
    dst.d2 = out->d2;
  }
  RadiusOut fill = dst;  // where k_radius<true> writes: storage order
  uint32_t* perm = nullptr;
  unsigned long long* keys_sorted = nullptr;
  if (sorted) {
    MH_TRY(ctx->build_b.reserve(5 * rb));
    char* st = ctx->build_b.as<char>();
    fill.gi = dst.gi ? (uint32_t*)st : nullptr;
    fill.x = dst.x ? (float*)(st + rb) : nullptr;
    fill.y = dst.y ? (float*)(st + 2 * rb) : nullptr;
    fill.z = dst.z ? (float*)(st + 3 * rb) : nullptr;
    fill.d2 = dst.d2 ? (float*)(st + 4 * rb) : nullptr;
    MH_TRY(ctx->build_c.reserve(nr * 8));
    MH_TRY(ctx->build_d.reserve(nr * 8));
    MH_TRY(ctx->build_e.reserve(nr * 4));
    fill.key = ctx->build_c.as<unsigned long long>();
    keys_sorted = ctx->build_d.as<unsigned long long>();
    perm = ctx->build_e.as<uint32_t>();
    tmp = 0;
    MH_HIP(rocprim::radix_sort_pairs(nullptr, tmp, fill.key, keys_sorted, rocprim::counting_iterator<uint32_t>(0), perm, (size_t)nr,
                                     0, 64, s));
    MH_TRY(ctx->sort_tmp.reserve(tmp));
  }
  hipLaunchKernelGGL(k_radius<true>, dim3(blocks), dim3(kRadiusBlock), 0, s, Ta, r2, rr, scan->x, scan->y, scan->z, (uint32_t)n, mv,
                     (uint32_t*)nullptr, (const uint32_t*)offsets, fill);
  MH_HIP(hipGetLastError());
  if (sorted) {
    // stable, and the input is in (query, storage position) order: ties in d2 keep the storage order
    tb = ctx->sort_tmp.bytes;
    MH_HIP(rocprim::radix_sort_pairs(ctx->sort_tmp.p, tb, fill.key, keys_sorted, rocprim::counting_iterator<uint32_t>(0), perm,
                                     (size_t)nr, 0, 64, s));
    hipLaunchKernelGGL(k_radius_gather, dim3(nblk(nr, kRadiusBlock)), dim3(kRadiusBlock), 0, s, (const uint32_t*)perm, (size_t)nr, fill,
                       dst);
    MH_HIP(hipGetLastError());
  }
  MH_HIP(mh::wait_stream(s));
  if (mem == MH_MEM_HOST) {
    if (out->global_idx) MH_HIP(hipMemcpy(out->global_idx, dst.gi, nr * 4, hipMemcpyDeviceToHost));
    if (out->gx) MH_HIP(hipMemcpy(out->gx, dst.x, nr * 4, hipMemcpyDeviceToHost));
    if (out->gy) MH_HIP(hipMemcpy(out->gy, dst.y, nr * 4, hipMemcpyDeviceToHost));
    if (out->gz) MH_HIP(hipMemcpy(out->gz, dst.z, nr * 4, hipMemcpyDeviceToHost));
    if (out->d2) MH_HIP(hipMemcpy(out->d2, dst.d2, nr * 4, hipMemcpyDeviceToHost));
  }
  return MH_OK;
}

mh_status mh_score_poses(const mh_map* map, const mh_scan* scan, const double* poses, size_t n_poses, double threshold,
                         double threshold_angular_deg, mh_pose_score* scores, int32_t mem) {
  // ---- refusals: all decided before anything is queued
  MH_REQUIRE(map && scan && scores && (poses || n_poses == 0), "null argument");
  MH_REQUIRE(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE, "bad mem space");
  MH_REQUIRE(map->ctx->device == scan->ctx->device, "map and scan live on different devices");
  MH_REQUIRE(isfinite(threshold) && threshold >= 1.0e-3 && threshold <= 1.0e3, "threshold must be finite and within [1e-3, 1e3] m");
  MH_REQUIRE(isfinite(threshold_angular_deg) && threshold_angular_deg >= 0.0, "angular threshold must be finite and >= 0");
  if (n_poses > (size_t)MH_SCORE_MAX_POSES)
    return fail(MH_ERR_UNSUPPORTED, "mh_score_poses: %zu poses exceed MH_SCORE_MAX_POSES (%d)", n_poses, MH_SCORE_MAX_POSES);
  for (size_t c = 0; c < n_poses; c++) MH_REQUIRE(pose_finite(poses + 12 * c), "non-finite pose");
  MH_REQUIRE(scan->n < 0xFFFFFFFFull, "scan size does not fit 32 bits");
  const Switches sw = read_switches();

  mh_ctx* ctx = scan->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t n = scan->n;
  if (n_poses == 0) return MH_OK;
  const size_t sbytes = n_poses * sizeof(mh_pose_score);
  if (n == 0) {  // zeroed scores
    if (mem == MH_MEM_HOST) {
      memset(scores, 0, sbytes);
    } else {
      MH_HIP(hipMemsetAsync(scores, 0, sbytes, s));
      MH_HIP(mh::wait_stream(s));
    }
    return MH_OK;
  }
  MH_TRY(map_ready_on(map, s));

  const float thr2 = (float)(threshold * threshold);  // the squares taken in fp64, rounded once (mh_nn_search)
  const double ang = threshold_angular_deg * 3.14159265358979323846 / 180.0;
  const float ang2 = (float)(ang * ang);
  const float qscale = (float)(1048576.0 / (double)thr2);
  const MapView mv = map->view(sw);

  // the poses travel in one copy; host-bound scores are summed in a staging block
  MH_TRY(ctx->staging.reserve(n_poses * 12 * sizeof(double)));
  MH_TRY(stage_in(ctx, ctx->staging, 0, poses, n_poses * 12 * sizeof(double), MH_MEM_HOST));
  const double* d_poses = ctx->staging.as<double>();
  mh_pose_score* d_scores = scores;
  if (mem == MH_MEM_HOST) {
    MH_TRY(ctx->compact.reserve(sbytes));
    d_scores = ctx->compact.as<mh_pose_score>();
  }
  MH_HIP(hipMemsetAsync(d_scores, 0, sbytes, s));
  // one workgroup per (candidate, tile), flattened; launches of at most 2^30 workgroups
  const uint32_t n_tiles = nblk(n, kScoreBlock);
  const size_t per_launch = std::max<size_t>(1, (size_t(1) << 30) / n_tiles);
  for (size_t c0 = 0; c0 < n_poses; c0 += per_launch) {
    const size_t nc = std::min(per_launch, n_poses - c0);
    hipLaunchKernelGGL(k_score_poses, dim3((uint32_t)(nc * n_tiles)), dim3(kScoreBlock), 0, s, d_poses + 12 * c0, n_tiles, scan->x,
                       scan->y, scan->z, (uint32_t)n, mv, thr2, ang2, qscale, d_scores + c0);
    MH_HIP(hipGetLastError());
  }
  if (mem == MH_MEM_HOST) MH_HIP(hipMemcpyAsync(scores, d_scores, sbytes, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
