// mh_icp.hip -- the hot path: correspondence search, residual/Jacobian accumulation, 6x6 Gauss-Newton
// solve and the ICP outer loop, all on the device (gfx950).
//
// Stands in for (all [U] = upstream classes the reference selects by name):
//   mp2p_icp::ICP::align                                   <- LidarOdometry.cpp:961-962
//   mp2p_icp::Matcher_Points_DistanceThreshold              <- lidar3d-default.yaml:195-204
//   mola::HashedVoxelPointCloud::nn_single_search           <- lidar3d-default.yaml:228-242
//   mp2p_icp::Solver_GaussNewton / optimal_tf_gauss_newton  <- lidar3d-default.yaml:184-190
//   mp2p_icp::QualityEvaluator_PairedRatio                  <- lidar3d-default.yaml:206-209
//   mp2p_icp::covariance                                    <- LidarOdometry.cpp:1009
//
// ONE translation unit (a __global__ kernel is defined where it is launched), in units:
//   mh_nn_device.h, mh_nn_flat.h   the searches: quad / row / k-best (branch and bound through the caches), plan / scan
//   mh_icp_types.h                 state and parameter blocks, the lock-step job descriptor, workgroup reductions
//   mh_k_match.h, mh_k_match_rows.h, mh_k_accum.h, mh_k_solve.h, mh_k_step.h (+ mh_loop_wave.h), mh_k_cov.h, mh_k_pairs.h
//                                  kernel bodies: matchers, accumulation, Gauss-Newton step + loop tail, the small layer's loops, covariance, pairings
//   mh_k_launch.h                  their __global__ entry points (single alignment | one job per blockIdx.y)
//   this file                      AlignJob: the chain a layer takes, loop control (one-launch loop | streaming | chunks + hipGraph), mh_icp_align
//   mh_icp_job.inl                 what AlignJob and LayersJob share: result / state / solver set-up, graph cache, result read-back
//   mh_k_layers.h, mh_k_claim.h, mh_k_match_kbest.h, mh_k_match_planes.h
//                                  the multi-layer loop's kernels: pair table, unique pairs, pairingsPerPoint > 1, plane pairs (KNN + PCA)
//   mh_icp_layers.inl, mh_icp_layers_batch.inl   LayersView (one job description), check_layers_job, LayersJob; the single call and the
//                                  lock-step batch behind mh_icp_align_layers* and mh_icp_align_layers_batch*
//   mh_icp_batch.inl               mh_icp_align_batch (lock-step groups)
//   mh_icp_api.inl                 matcher- / solver-granular entry points (mh_nn_search*, mh_gn_solve, mh_covariance)
//
// Kernel sequence per ICP iteration of a LARGE layer (everything stays in HBM/L2; the host never sees pairings):
//   k_match_flat     a wave per 64 scan points: transform, exact bounded search (plan / scan), threshold test, store pairing
//   k_accum          robust weight + 18 fp64 moment sums of the stored pairings at the current pose -> partials
//   k_solve          one workgroup: ordered sum of partials, prior factor, LDL^T, T <- T(+)exp(delta),
//                    inner/outer loop bookkeeping, stall + hook tests, termination flag, next threshold
//   k_accum, k_solve (inner Gauss-Newton steps >= 1 on the SAME pairings)
// Smaller layers take shorter chains (chosen by size in plan_alignment, run by AlignJob):
//   <= 32 k points   k_match16: a DPP row (16 lanes) per point; up to 12 k points it also accumulates the first step
//   <= 8 k points    k_step16 x max_inner: search + sums per launch, the Gauss-Newton step carried into the next launch
//   <= 2560 points   k_icp16: the whole loop in ONE launch (single alignments); lock-step batches of point layers up to 4096
//                    points: k_icpw_b (the same loop with the plan / scan search) -- lidar3d-default.yaml's ICP layer
//   NDT maps         Matcher_Point2Plane rides in the row kernels (k_step16<true>, k_icp16<true>, k_match16<true,.>), its rows are
//                    summed alongside (k_accum_both); above 32 k points k_match_pl (one lane per point)
// No fp atomics anywhere: reductions are fixed-shape trees, so results are bitwise reproducible.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <new>
#include <type_traits>
#include <vector>

#include "mh_nn_device.h"
#include "mh_nn_flat.h"

#include "mh_icp_types.h"
#include "mh_k_match.h"
#include "mh_k_accum.h"
#include "mh_k_match_rows.h"
#include "mh_k_solve.h"
#include "mh_k_step.h"
#include "mh_k_cov.h"
#include "mh_k_launch.h"
#include "mh_k_layers.h"
#include "mh_k_claim.h"
#include "mh_k_match_kbest.h"
#include "mh_k_match_planes.h"
#include "mh_k_pairs.h"

// ================================================================================================
// Host side
// ================================================================================================
namespace {

inline uint32_t nblk(size_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }


// One device block [state | parameters] with a pinned mirror of the same layout: an alignment starts with ONE upload.
constexpr size_t kParamsOffset = (sizeof(IcpDeviceState) + 255) / 256 * 256;
// The threshold schedules of a single alignment (threshold | kernel_param | pt2pl_threshold, max_iterations doubles each) ride
// behind the parameters in the same block when they fit: state, parameters and schedules go up in ONE copy instead of two.
constexpr size_t kInlineSchedDoubles = 3 * 400;
constexpr size_t kInlineSchedOffset = (kParamsOffset + sizeof(IcpDeviceParams) + 63) / 64 * 64;

mh_status ensure_state(mh_ctx* ctx) {
  if (!ctx->d_state) {
    char *d = nullptr, *h = nullptr;
    const size_t second_off = (kInlineSchedOffset + kInlineSchedDoubles * sizeof(double) + 255) / 256 * 256;  // k_step16's two ping-pong state blocks (heads only)
    MH_HIP(hipMalloc((void**)&d, second_off + 2 * 256));
    static_assert(kStateHeadDwords * 4 <= 256, "a ping-pong block per 256 bytes");
    const size_t prog_off = ((kInlineSchedOffset + kInlineSchedDoubles * sizeof(double) + 127) / 128) * 128;  // a cache line of its own
    MH_HIP(hipHostMalloc((void**)&h, prog_off + 128, hipHostMallocDefault));
    ctx->d_state = (IcpDeviceState*)d;
    ctx->d_state_b = (IcpDeviceState*)(d + second_off);
    ctx->h_state = (IcpDeviceState*)h;
    ctx->d_params = (IcpDeviceParams*)(d + kParamsOffset);
    ctx->h_params = (IcpDeviceParams*)(h + kParamsOffset);
    // the word the device loop publishes its progress in (run_streaming): page-locked host memory, written by the kernels
    ctx->h_progress = (uint32_t*)(h + prog_off);
    *ctx->h_progress = 0;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, ctx->h_progress, 0) != hipSuccess) dp = nullptr;  // (then the loop is never streamed)
    ctx->d_progress = (uint32_t*)dp;
  }
  return MH_OK;
}

// state + parameters (+ the schedules that ride behind them: inline_sched doubles) in one copy (start of mh_icp_align)
mh_status upload_state_and_params(mh_ctx* ctx, const MatchK& mk, const SolveK& sk, size_t inline_sched = 0) {
  ctx->h_params->mk = mk;
  ctx->h_params->sk = sk;
  const size_t bytes = inline_sched ? kInlineSchedOffset + inline_sched * sizeof(double) : kParamsOffset + sizeof(IcpDeviceParams);
  MH_HIP(hipMemcpyAsync(ctx->d_state, ctx->h_state, bytes, hipMemcpyHostToDevice, ctx->stream));
  return MH_OK;
}
// parameters -> pinned mirror -> device block (the caller has synchronised the previous use of the mirror)
mh_status upload_params(mh_ctx* ctx, const MatchK& mk, const SolveK& sk) {
  ctx->h_params->mk = mk;
  ctx->h_params->sk = sk;
  MH_HIP(hipMemcpyAsync(ctx->d_params, ctx->h_params, sizeof(IcpDeviceParams), hipMemcpyHostToDevice, ctx->stream));
  return MH_OK;
}

mh_status ensure_pair_buffers(mh_ctx* ctx, size_t n) {
  const size_t nn = n ? n : 1;
  MH_TRY(ctx->pair_q.reserve(nn * sizeof(float4)));
  MH_TRY(ctx->pair_gidx.reserve(nn * sizeof(uint32_t)));
  const size_t nb = nblk(nn);
  MH_TRY(ctx->partials.reserve((size_t)kGenN * nb * sizeof(double)));
  return MH_OK;
}

mh_status ensure_pl_buffers(mh_ctx* ctx, size_t n) {
  const size_t nn = n ? n : 1;
  MH_TRY(ctx->pl_c.reserve(nn * sizeof(float4)));
  MH_TRY(ctx->pl_n.reserve(nn * sizeof(float4)));
  MH_TRY(ctx->partials_b.reserve((size_t)kGenN * nblk(nn) * sizeof(double)));
  return MH_OK;
}

void init_state(IcpDeviceState* h, const double T[12]) {
  memset(h, 0, sizeof(*h));
  for (int i = 0; i < 12; i++) {
    h->T[i] = T[i];
    h->T_prev[i] = T[i];
  }
  h->solver_ok = 1;
  for (int i = 0; i < 6; i++) h->cov[i * 7] = 1e6;
}

void fill_prior(SolveK& k, const mh_prior* prior) {
  k.has_prior = prior ? 1u : 0u;
  if (!prior) return;
  Pose P;
  for (int i = 0; i < 12; i++) P.m[i] = prior->mean[i];
  const Pose Pi = inverse(P);
  for (int i = 0; i < 12; i++) k.prior_mean_inv[i] = Pi.m[i];
  for (int i = 0; i < 36; i++) k.prior_info[i] = prior->info[i];
}

bool pose_ok(const double T[12]) {
  for (int i = 0; i < 12; i++)
    if (!isfinite(T[i])) return false;
  return true;
}

// compaction of pairing buffers (gidx / q, n entries) into caller arrays; returns the number of pairs
mh_status compact_pairs_of(mh_ctx* ctx, const uint32_t* gidx, const float4* q, size_t n, const mh_pairs_out* out, int32_t mem,
                           uint64_t* n_pairs_out) {
  hipStream_t s = ctx->stream;
  const uint32_t nb = nblk(n);
  const size_t n4 = ((n + 63) / 64) * 64;
  // layout: counts[nb] | offsets[nb] | total[1] | (host staging) li,gi,x,y,z,d2 [n4 each]
  const size_t hdr = (((size_t)2 * nb + 1) * 4 + 255) / 256 * 256;
  MH_TRY(ctx->compact.reserve(hdr + 6 * n4 * 4));
  uint32_t* counts = ctx->compact.as<uint32_t>();
  uint32_t* offsets = counts + nb;
  uint32_t* total = offsets + nb;
  char* stage = ctx->compact.as<char>() + hdr;
  uint32_t *o_li, *o_gi;
  float *o_x, *o_y, *o_z, *o_d2;
  if (mem == MH_MEM_DEVICE) {
    o_li = out->local_idx; o_gi = out->global_idx; o_x = out->gx; o_y = out->gy; o_z = out->gz; o_d2 = out->d2;
  } else {
    o_li = out->local_idx ? (uint32_t*)(stage) : nullptr;
    o_gi = out->global_idx ? (uint32_t*)(stage + n4 * 4) : nullptr;
    o_x = out->gx ? (float*)(stage + 2 * n4 * 4) : nullptr;
    o_y = out->gy ? (float*)(stage + 3 * n4 * 4) : nullptr;
    o_z = out->gz ? (float*)(stage + 4 * n4 * 4) : nullptr;
    o_d2 = out->d2 ? (float*)(stage + 5 * n4 * 4) : nullptr;
  }
  uint32_t h_total = 0;
  if (n) {
    hipLaunchKernelGGL(k_count_valid, dim3(nb), dim3(kBlock), 0, s, gidx, (uint32_t)n, counts);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, counts, nb, offsets, total);
    hipLaunchKernelGGL(k_compact, dim3(nb), dim3(kBlock), 0, s, gidx, q, (uint32_t)n, offsets, o_li, o_gi, o_x, o_y, o_z, o_d2);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h_total, total, 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
  }
  if (mem == MH_MEM_HOST && h_total) {
    const size_t b = (size_t)h_total * 4;
    if (out->local_idx) MH_HIP(hipMemcpy(out->local_idx, o_li, b, hipMemcpyDeviceToHost));
    if (out->global_idx) MH_HIP(hipMemcpy(out->global_idx, o_gi, b, hipMemcpyDeviceToHost));
    if (out->gx) MH_HIP(hipMemcpy(out->gx, o_x, b, hipMemcpyDeviceToHost));
    if (out->gy) MH_HIP(hipMemcpy(out->gy, o_y, b, hipMemcpyDeviceToHost));
    if (out->gz) MH_HIP(hipMemcpy(out->gz, o_z, b, hipMemcpyDeviceToHost));
    if (out->d2) MH_HIP(hipMemcpy(out->d2, o_d2, b, hipMemcpyDeviceToHost));
  }
  if (n_pairs_out) *n_pairs_out = h_total;
  return MH_OK;
}
// ... of the context's own pair buffers (a single alignment's)
mh_status compact_pairs(mh_ctx* ctx, size_t n, const mh_pairs_out* out, int32_t mem, uint64_t* n_pairs_out) {
  return compact_pairs_of(ctx, ctx->pair_gidx.as<uint32_t>(), ctx->pair_q.as<float4>(), n, out, mem, n_pairs_out);
}

// compaction of point-to-plane pairing buffers (pl_c / pl_n, n entries) into caller arrays
mh_status compact_pl_pairs_of(mh_ctx* ctx, const float4* pl_c, const float4* pl_n, size_t n, const mh_pairs_pl_out* out, int32_t mem,
                              uint64_t* n_pairs_out) {
  hipStream_t s = ctx->stream;
  const uint32_t nb = nblk(n);
  const size_t n4 = ((n + 63) / 64) * 64;
  // layout: flags[n4] | counts[nb] | offsets[nb] | total[1] | (host staging) li,cx,cy,cz,nx,ny,nz [n4 each]
  const size_t hdr = ((n4 + (size_t)2 * nb + 1) * 4 + 255) / 256 * 256;
  MH_TRY(ctx->compact.reserve(hdr + 7 * n4 * 4));
  uint32_t* flags = ctx->compact.as<uint32_t>();
  uint32_t* counts = flags + n4;
  uint32_t* offsets = counts + nb;
  uint32_t* total = offsets + nb;
  char* stage = ctx->compact.as<char>() + hdr;
  void* o[7] = {out->local_idx, out->cx, out->cy, out->cz, out->nx, out->ny, out->nz};
  void* d[7];
  for (int a = 0; a < 7; a++) d[a] = (mem == MH_MEM_DEVICE) ? o[a] : (o[a] ? (void*)(stage + (size_t)a * n4 * 4) : nullptr);
  uint32_t h_total = 0;
  if (n) {
    hipLaunchKernelGGL(k_pl_flags, dim3(nb), dim3(kBlock), 0, s, pl_c, (uint32_t)n, flags);
    hipLaunchKernelGGL(k_count_valid, dim3(nb), dim3(kBlock), 0, s, flags, (uint32_t)n, counts);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, counts, nb, offsets, total);
    hipLaunchKernelGGL(k_compact_pl, dim3(nb), dim3(kBlock), 0, s, flags, pl_c, pl_n,
                       (uint32_t)n, offsets, (uint32_t*)d[0], (float*)d[1], (float*)d[2], (float*)d[3], (float*)d[4],
                       (float*)d[5], (float*)d[6]);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h_total, total, 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
  }
  if (mem == MH_MEM_HOST && h_total)
    for (int a = 0; a < 7; a++)
      if (o[a]) MH_HIP(hipMemcpy(o[a], d[a], (size_t)h_total * 4, hipMemcpyDeviceToHost));
  if (n_pairs_out) *n_pairs_out = h_total;
  return MH_OK;
}

// the argument rules of the KNN + PCA plane matcher (mh_nn_search_pt2pl_knn; a plane pair of mh_icp_align_layers_planes obeys the
// same) and its kernel argument
mh_status check_pl_knn_params(const mh_pt2pl_knn_params* params) {
  MH_REQUIRE(params->knn >= 3 && params->knn <= (uint32_t)kMaxPlaneKnn, "knn must be 3..MH_MAX_PLANE_KNN");
  MH_REQUIRE(isfinite(params->distance_threshold) && isfinite(params->plane_eigen_threshold) && isfinite(params->search_radius) &&
             params->search_radius > 0.0, "bad thresholds");
  return MH_OK;
}
PlKnnArg pl_knn_arg(const mh_pt2pl_knn_params* params) {
  PlKnnArg a;
  a.distance_threshold = params->distance_threshold;
  a.plane_eigen_threshold = params->plane_eigen_threshold;
  a.radius2 = (float)(params->search_radius * params->search_radius);
  a.knn = params->knn;
  a.min_pts = params->minimum_plane_points < 3u ? 3u : params->minimum_plane_points;  // (three points span a plane)
  return a;
}

std::atomic<unsigned long long> g_loop16_runs{0}, g_loop16_fallbacks{0};  // one-launch loops started / abandoned for the chain (mh_debug_loop_stats)
// plan / scan matcher launches that went to the device (mh_debug_flat_stats): k_match_flat<true> | <false> | k_match_flat_b<true> |
// <false>.  Counted where a launch is issued; the launches a captured chunk holds are counted on every replay (enqueue_cached).
std::atomic<unsigned long long> g_flat_launches[4];
inline void count_flat_launches(uint32_t which, uint32_t k) {
  if (k) g_flat_launches[which].fetch_add(k, std::memory_order_relaxed);
}
uint32_t loop_cu_limit(const Switches& sw, int device) {
  static uint32_t cap[64] = {0};
  uint32_t& cu = cap[(unsigned)device % 64u];
  if (!cu) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 64;
    cu = (uint32_t)v;
  }
  return sw.loop16_cus >= 0 ? (uint32_t)sw.loop16_cus : cu;  // (MH_LOOP16_CUS: test knob of the admission limit)
}
// the loops of `callers` alignments of `ng` groups each fit 70 % of the device's CUs side by side (one group per workgroup; shared
// loops whose workgroups take 2 or 4 groups each were measured for 6 / 8 / 16 callers and lost to lock-step batches: 3100-3550 /
// 3260-3540 / 3000-3140 against 4960 / 5300 / 5470-6150 scans/s -- the callers' other kernels start and stop beside them)
// Admission is counted in HALF compute units: a k_icp16 workgroup (512 lanes x ~250 registers) takes a CU, a k_icpw workgroup
// (256 lanes, 63 KB of LDS) half of one.
constexpr uint32_t kLoopUnitsPerCu = 2;
// MH_LOOPW = all | solo | batch | none: where k_icpw / k_icpw_b (plan / scan search, 128 points per workgroup) replace k_icp16 /
// k_icp16_b (a DPP row per point) on point layers.  (MH_NO_LOOPW=1 = none.)
bool loop_wave_enabled(const Switches& sw, bool batch) {
  return !sw.no_loopw && (sw.loopw == 'a' || sw.loopw == (batch ? 'b' : 's'));
}
bool loops_fit(const Switches& sw, int device, uint32_t units, uint32_t callers) {
  // (and never more than MH_SOLO_MAX_CALLERS, 4: beyond, every measurement so far says lock-step batches -- the loops' own
  //  streams share four hardware queues with everything else the callers issue, and a loop holds its queue for 0.5 ms)
  return callers <= 1 || (callers <= sw.solo_max_callers &&
                          (uint64_t)callers * units * 10u <= (uint64_t)loop_cu_limit(sw, device) * kLoopUnitsPerCu * 7u);
}

// Admission of one-launch loops: the workgroups of all loops running on a device must be resident together (a loop's
// workgroups wait for each other), so their sum stays below the CU count less a reserve for what else is running; kernels
// that merely pass through (other sequences' large layers, map updates) delay a loop's start, they cannot block it.
std::atomic<uint32_t>& loop_count(int device) {
  static std::atomic<uint32_t> c[64];
  return c[(unsigned)device % 64u];
}
// arm > 0: a loop was abandoned; arm < 0: a loop ran to its end; 0: true while the hold-off lasts (counts down).  The hold-off
// doubles with every abandonment in a row (200, 400, ... 12 800 alignments): on a device shared with other processes a loop's
// workgroups may never run together, and every attempt costs its 20 ms limit (MH_NO_LOOP16=1 is the switch for such
// a deployment).
bool loop_holdoff(int device, int arm) {
  static std::atomic<int> left[64], streak[64];
  std::atomic<int>& v = left[(unsigned)device % 64u];
  std::atomic<int>& st = streak[(unsigned)device % 64u];
  if (arm > 0) {
    const int k = st.fetch_add(1);
    v.store(200 << (k < 6 ? k : 6));
    return true;
  }
  if (arm < 0) {
    st.store(0);
    return false;
  }
  int cur = v.load();
  while (cur > 0)
    if (v.compare_exchange_weak(cur, cur - 1)) return true;
  return false;
}
// The units one or several loops hold of a device's admission count, given back by release() or, whatever way the call that
// took them ends, by the destructor.
class LoopAdmission {
 public:
  LoopAdmission() = default;
  LoopAdmission(LoopAdmission&& o) noexcept : device_(o.device_), units_(o.units_) { o.units_ = 0; }  // (move-only)
  ~LoopAdmission() { release(); }
  // `units` half CUs of `device` (an empty guard only): true once they are held
  bool admit(const Switches& sw, int device, uint32_t units) {
    const uint32_t limit = loop_cu_limit(sw, device) * kLoopUnitsPerCu;
    if (units > limit) return false;
    // A loop that does not fit now waits for the running ones (each takes a fraction of a millisecond) rather than fall back to
    // the chain, whose forty-odd launches would queue behind the same loops: eight sequences of the default pipeline keep five
    // loops on the device at any time.  MH_LOOP16_WAIT_US (2000): how long before the chain is taken after all.
    std::atomic<uint32_t>& c = loop_count(device);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
      uint32_t cur = c.load();
      while (cur + units <= limit)
        if (c.compare_exchange_weak(cur, cur + units)) {
          device_ = device;
          units_ = units;
          return true;
        }
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= sw.loop16_wait_us)
        return false;
      if (spins < 64) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
  }
  void release() {
    if (units_) loop_count(device_).fetch_sub(units_);
    units_ = 0;
  }
 private:
  int device_ = 0;
  uint32_t units_ = 0;
};

// The correspondence kernel of the fused loop, MH_MATCH=<letter> (all exact, bit-identical pairings).  The numbers go into the
// graph-cache key and the debug prints.
enum class Matcher : int {
  Point = 0,    // "p": one lane per point, branch-and-bound, fused accumulation                            -> k_match<true, 1>
  Literal = 1,  // "x": one lane per point, the literal 27-voxel scan of the reference (A/B baseline)        -> k_match<true, 0>
  Quad = 4,     // "q": a DPP quad per scan point, merged candidate scans (the default of rounds 1-4)        -> k_match4 + k_accum
  Row = 5,      // "s": a DPP row (16 lanes) per point (default up to kRowMaxPoints)                         -> k_match16 + k_accum
  Flat = 9,     // "f": plan / scan (mh_nn_flat.h; default above kRowMaxPoints): a wave per 64 points, per-point / per-voxel /
                //      per-record work each on all 64 lanes                                                  -> k_match_flat + k_accum
};  // (6, 7, 8 were "t", "w", "o": the tile / wave / sorted-scan matchers, removed -- profiles/r02_tile_matcher.md; the letters are refused)
// the one-lane matchers sum the first Gauss-Newton step themselves; every other one leaves it to k_accum (or the row kernel)
inline bool one_lane(Matcher m) { return m == Matcher::Point || m == Matcher::Literal; }

enum class Loop { None, Icp16, Icpw };  // one-launch loop: k_icp16 (a DPP row per point) | k_icpw (plan / scan search)
struct AlignPlan {
  Matcher matcher = Matcher::Row;
  char retired = 0;         // MH_MATCH names a matcher that was removed ("t", "w", "o"): start() fails
  bool fused16 = false;     // the row kernel accumulates the first Gauss-Newton step itself (layers above the one-workgroup size)
  bool step_chain = false;  // k_step16 launches (row-kernel layers up to kStepMaxPoints)
  bool streaming = false;   // run_streaming(): iterations enqueued one by one behind the device's published progress
  Loop loop = Loop::None;   // the one-launch loop that takes the streaming chain's place if the hold-off and admission allow ...
  uint32_t loop_units = 0;  // ... and the half CUs it holds meanwhile (0: the layer is too large for it)
};

// The path of one alignment, from the switches and its shape alone (no HIP call, no admission): AlignJob::start runs it,
// mh_icp_align_prefers_solo promises it and a batch groups its jobs by it.  `map` null: the map-dependent downgrades are left out
// (they never touch the row matcher).  `auto_control`: a single alignment with automatic polling on a context with a progress word.
AlignPlan plan_alignment(const Switches& sw, size_t n, bool pl, uint32_t matched_points, const mh_map* map, bool prof,
                         bool auto_control) {
  AlignPlan a;
  a.matcher = n <= kRowMaxPoints ? Matcher::Row : Matcher::Flat;
  switch (sw.match) {
    case 'f': a.matcher = Matcher::Flat; break;
    case 'q': a.matcher = Matcher::Quad; break;
    case 's': a.matcher = Matcher::Row; break;
    case 'p': a.matcher = Matcher::Point; break;
    case 'x': a.matcher = Matcher::Literal; break;
    case 't': case 'w': case 'o': a.retired = sw.match; a.matcher = Matcher::Flat; break;
  }
  if (map && a.matcher == Matcher::Literal && map->view(sw).ndt) a.matcher = Matcher::Point;  // "x" walks contiguous z-runs; NDT maps interleave statistics records
  // MH_MATCHED_POINTS_SKIP (U12): the point matcher has to know the plane matcher's verdict for the same point -- the row
  // kernel runs both in one launch (k_match16<true>), whatever the layer's size
  if (pl && matched_points == MH_MATCHED_POINTS_SKIP) a.matcher = Matcher::Row;
  if (map && a.matcher == Matcher::Flat && map->pts.bytes / sizeof(float4) >= kFlatMaxRecords) a.matcher = Matcher::Quad;  // (the chunk word holds 30 bits of record index)
  // (measured per iteration, fused vs k_accum: 31.0 vs 33.8 us at 4 k points, 33.2 vs 35.0 at 8 k, equal at 16 k,
  //  45.9 vs 41.8 at 32 k -- one partial row per 16 points makes the solve's reduction the longer pole there)
  a.fused16 = a.matcher == Matcher::Row && !pl && n <= kFused16MaxPoints && !sw.no_fuse16;
  // profiled jobs time the match kernel alone: they, and MH_NO_STEP_CHAIN=1, take the chains with a match kernel of its own
  a.step_chain = a.matcher == Matcher::Row && n <= kStepMaxPoints && !prof && !sw.no_step_chain;
  // Streaming loop control (single alignments with automatic polling): instead of a predicted chunk of iterations whose
  // unused tail idles on the stream (27.8 iterations' worth of kernels enqueued for 21 executed on the city drive, plus
  // 0.64 extra host round trips per scan), the host follows the progress word the solve kernels publish and keeps
  // kStreamLead (2) iterations queued ahead.  Not for lock-step batches, profiled jobs, or when switched off (MH_NO_STREAM=1).
  a.streaming = auto_control && !prof && !sw.no_stream;
  // k_icp16: where the streaming chain would run and the layer has at most kLoopMaxGroups groups (k_icpw: kLwMaxGroups)
  if (a.streaming && a.step_chain && !sw.no_loop16) {
    const bool wave = !pl && loop_wave_enabled(sw, false);
    const uint32_t ng = (uint32_t)((n + kStepPoints - 1) / kStepPoints);
    a.loop = wave ? Loop::Icpw : Loop::Icp16;
    if (ng <= (wave ? kLwMaxGroups : kLoopMaxGroups)) a.loop_units = wave ? (ng + kLwGroups - 1) / kLwGroups : kLoopUnitsPerCu * ng;
  }
  return a;
}

// Loop control constants (MH_STREAM_LEAD, MH_CHUNK_MARGIN and MH_CHUNK_NEXT were their A/B switches)
constexpr uint32_t kStreamLead = 2;   // iterations a streaming alignment keeps queued ahead of the device's published one
constexpr uint32_t kChunkMargin = 2;  // iterations the first chunk adds to the expected count
constexpr uint32_t kChunkNext = 6;    // iterations of the chunks after the first (automatic polling)

#include "mh_icp_job.inl"  // set-up, graph cache and read-back shared with LayersJob

// One alignment in flight on one context: enqueue / poll state machine shared by mh_icp_align and
// mh_icp_align_batch.
struct AlignJob {
  const mh_map* map = nullptr;
  const mh_scan* scan = nullptr;
  mh_ctx* ctx = nullptr;
  const mh_icp_params* p = nullptr;
  mh_icp_result* res = nullptr;
  mh_icp_iter* trace = nullptr;
  MatchK mk{};
  SolveK sk{};
  uint32_t nb = 0, nbm = 0, nba = 0, enqueued = 0, chunk = 0, prof_n = 0, polls = 0, kind = 0;
  uint32_t step_total = 0;  // ... launches of the chunks enqueued so far when they are replayed from a graph (step_launches only counts direct launches)
  uint32_t serial_base = 0, step_launches = 0;  // k_step16's hand-over: the state block's serial number at upload, launches since
  // k_step16 chain: the state block the next launch reads (2 = the canonical one: after the upload and after a close-only launch;
  // 0 / 1 = the ping-pong pair) and the half of the partials it reads
  uint32_t step_src = 2, step_ppar = 0;
  bool auto_chunk = false;
  bool defer_upload = false;   // batches: the pinned mirrors are filled, the copies are issued by the batch (staged) or flush()
  size_t nsched_pending = 0;
  size_t inline_sched = 0;  // doubles of the schedules that ride behind the parameter block (single alignments; 0: their own copy)
  const Switches* sw = nullptr;  // the snapshot of the entry point that runs this job
  AlignPlan plan{};
  bool finished = false, trivial = false;
  bool prof = false;  // time this job's match kernels with events (then it cannot use the graph path)
  bool pl = false;    // Matcher_Point2Plane runs before the point matcher (lidar3d-ndt.yaml:195-210)
  bool streaming = false;  // run_streaming(): iterations are enqueued one by one behind the device's published progress
  bool skip_tail = false;  // ... and the covariance kernels + state read-back only once the loop has ended
  bool flat32 = false;     // Matcher::Flat: k_match_flat<true> (flat_off32 holds and MH_NO_OFF32 is off), decided once in start(); a word of the graph key
  bool loop16 = false;         // run_loop16(): the whole loop of a small layer in ONE launch (plan.loop: k_icp16 / k_icpw)
  bool forbid_loop16 = false;  // ... not for this job: the second attempt after a loop whose workgroups gave up
  LoopAdmission loop_adm;      // what this job holds of the device's admission count while its loop runs
  LoopExchange loop_x;         // ... its exchange block and serial numbers
  uint32_t loop_steps = 0;     // ... and the Gauss-Newton steps it may take

  uint64_t potential() const { return scan->n * (pl ? 2u : 1u); }  // every matcher adds its layer size (App.B U6)

  mh_status start(const Switches& switches, const mh_map* m, const mh_scan* sc, const mh_icp_params* prm, const double* T0,
                  const mh_prior* prior, mh_icp_result* r, mh_icp_iter* tr, size_t batch_index = 0) {
    sw = &switches; map = m; scan = sc; ctx = sc->ctx; p = prm; res = r; trace = tr;
    prof = prm->profile == 1 || (prm->profile == 2 && batch_index == 0);
    pl = prm->pt2pl_threshold != nullptr;
    if (begin_result(res, p, T0, potential())) {
      finished = trivial = true;
      return MH_OK;
    }
    MH_TRY(set_device(ctx));
    MH_TRY(ensure_state(ctx));
    MH_TRY(ensure_pair_buffers(ctx, scan->n));
    hipStream_t s = ctx->stream;
    MH_TRY(map_ready_on(map, s));  // a key-frame update still running on the map's side stream (mh_map_insert)
    const size_t mi = p->max_iterations;
    if (pl) {
      if (!map->view(*sw).ndt)
        return fail(MH_ERR_INVALID_ARGUMENT, "pt2pl_threshold given but the map carries no NDT statistics "
                                             "(build it with ndt_max_eigen_ratio > 0)");
      MH_TRY(ensure_pl_buffers(ctx, scan->n));
    }
    MH_TRY(ctx->sched.reserve(3 * mi * sizeof(double)));
    {  // threshold | kernel_param | pt2pl_threshold schedules: packed in a pinned staging block, one upload
      const size_t nsched = (pl ? 3 : 2) * mi;
      MH_TRY(ctx->h_sched.reserve(3 * mi * sizeof(double)));
      double* const h_sched = ctx->h_sched.as<double>();
      memcpy(h_sched, p->threshold, mi * sizeof(double));
      memcpy(h_sched + mi, p->kernel_param, mi * sizeof(double));
      if (pl) {  // MH_PT2PL_CENTROID_DISTANCE travels as a negative threshold (pl_accept)
        const double sgn = p->pt2pl_mode == MH_PT2PL_CENTROID_DISTANCE ? -1.0 : 1.0;
        for (size_t k = 0; k < mi; k++) h_sched[2 * mi + k] = sgn * fabs(p->pt2pl_threshold[k]);
      }
      nsched_pending = nsched;
      // a single alignment whose schedules fit behind the parameter block: they travel with it (one copy, below)
      inline_sched = (!defer_upload && nsched <= kInlineSchedDoubles) ? nsched : 0;
      if (inline_sched)
        memcpy(reinterpret_cast<char*>(ctx->h_state) + kInlineSchedOffset, h_sched, nsched * sizeof(double));
      else if (!defer_upload)
        MH_HIP(hipMemcpyAsync(ctx->sched.p, h_sched, nsched * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (trace) MH_TRY(ctx->trace.reserve(mi * sizeof(mh_icp_iter)));
    const double ang = p->threshold_angular_deg * 3.14159265358979323846 / 180.0;
    serial_base = begin_state(ctx, T0, p->threshold[0], (float)(ang * ang), p->kernel_param[0]);  // uploaded together with the parameters below
    step_launches = 0;
    step_total = 0;

    double* const sched_dev = inline_sched ? reinterpret_cast<double*>(reinterpret_cast<char*>(ctx->d_state) + kInlineSchedOffset)
                                           : ctx->sched.as<double>();
    mk.thr = sched_dev;
    mk.kparam = sched_dev + mi;
    mk.ang2 = (float)(ang * ang);
    mk.kernel = p->gn.robust_kernel;
    mk.w_pt2pt = p->gn.weight_pt2pt;
    mk.w_pt2pl = p->gn.weight_pt2pl;
    mk.pl_thr = pl ? sched_dev + 2 * mi : nullptr;
    mk.skip_pl_paired = (pl && p->matched_points == MH_MATCHED_POINTS_SKIP) ? 1u : 0u;
    sk = make_solve_params(p, prior, mk, trace ? ctx->trace.as<mh_icp_iter>() : nullptr);
    plan = plan_alignment(*sw, scan->n, pl, p->matched_points, map, prof,
                          p->poll_every == 0 && !defer_upload && ctx->d_progress != nullptr);
    if (plan.retired)
      return fail(MH_ERR_INVALID_ARGUMENT, "MH_MATCH=%c names a matcher that was retired (the tile / wave / sorted-scan matchers): no build has it", plan.retired);
    const Matcher mt = plan.matcher;
    streaming = plan.streaming;
    sk.host_progress = streaming ? ctx->d_progress : nullptr;
    nb = nblk(scan->n);
    if (mt == Matcher::Quad || mt == Matcher::Flat) {  // nn_search_quad / the plan-scan matcher read the map's sub-voxel index
      MH_TRY(map_ensure_qidx(*sw, map, ctx->stream));
      if (!map->view(*sw).pts_q) return fail(MH_ERR_INTERNAL, "the map's sub-voxel index is missing (matcher variant %d needs it)", (int)mt);
    }
    flat32 = mt == Matcher::Flat && !sw->no_off32 && flat_off32(map, scan->n);  // (after map_ensure_qidx: pts_q has its size)
    nba = nblk_acc(scan->n);
    // who writes the partials of the first Gauss-Newton step: the row kernel (16 points per workgroup), k_accum, or k_match
    nbm = plan.fused16 ? (uint32_t)((16ull * scan->n + kBlock - 1) / kBlock) : (one_lane(mt) ? nb : nba);
    MH_TRY(ctx->partials.reserve((size_t)kGenN * (nbm > nb ? nbm : nb) * sizeof(double)));
    if (mt == Matcher::Row && scan->n <= kStepMaxPoints) {  // k_step16: two halves of one column per group of 32 points
      const size_t ng = (scan->n + kStepPoints - 1) / kStepPoints;
      MH_TRY(ctx->partials.reserve(2 * (size_t)kStepRowsA * (ng ? ng : 1) * sizeof(double)));
      if (pl) MH_TRY(ctx->partials_b.reserve(2 * (size_t)kStepRowsB * (ng ? ng : 1) * sizeof(double)));
    }
    step_src = 2;
    step_ppar = 0;
    // the one-launch loop if the workgroups of all loops running on this device still fit its CUs (every workgroup of a loop
    // has to be resident while it runs); otherwise the chain, bit for bit the same result.  (After a loop had to be abandoned --
    // somebody else's work kept its workgroups from running together, ~0.1 s lost -- the next 200 alignments on the device take
    // the chain before another loop is tried.)
    loop16 = plan.loop != Loop::None && !forbid_loop16 && !loop_holdoff(ctx->device, 0) && plan.loop_units &&
             loop_adm.admit(*sw, ctx->device, plan.loop_units);
    if (loop16) {
      streaming = false;
      sk.host_progress = nullptr;
      if (plan.loop == Loop::Icpw) {  // the plan / scan search reads the map's sub-voxel index (built once per map content, on this stream)
        MH_TRY(map_ensure_qidx(*sw, map, ctx->stream));
        if (!map->view(*sw).pts_q) return fail(MH_ERR_INTERNAL, "the map's sub-voxel index is missing (k_icpw needs it)");
      }
      // (MH_LOOP16_TEST_ABANDON: the loop is cut short as if its workgroups had given up -- the caller's second attempt is what is tested)
      loop_steps = sw->loop16_test_abandon ? 1u : p->max_iterations * p->gn.max_inner_iterations + 1u;
      MH_TRY(loop_exchange(ctx, s, loop_steps, loop_x));
    }
    if (defer_upload) {
      ctx->h_params->mk = mk;
      ctx->h_params->sk = sk;
    } else {
      MH_TRY(upload_state_and_params(ctx, mk, sk, inline_sched));
    }
    auto_chunk = p->poll_every == 0;
    kind = 0;
    chunk = first_chunk(p, ctx->predicted_iterations[kind]);
    polls = 0;
    enqueued = 0;
    prof_n = 0;
    if (prof) {
      const uint32_t need = 2 * p->max_iterations;
      if (ctx->prof_cap < need) {
        hipEvent_t* ne = new (std::nothrow) hipEvent_t[need];
        if (!ne) return fail(MH_ERR_OUT_OF_MEMORY, "host allocation failed");
        for (uint32_t i = 0; i < ctx->prof_cap; i++) ne[i] = ctx->prof_ev[i];
        for (uint32_t i = ctx->prof_cap; i < need; i++) MH_HIP(hipEventCreate(&ne[i]));
        delete[] ctx->prof_ev;
        ctx->prof_ev = ne;
        ctx->prof_cap = need;
      }
      MH_HIP(hipEventRecord(ctx->ev_t0, s));
    }
    return MH_OK;
  }

  // issues the copies a deferred start() left out, on this job's own stream
  mh_status flush_deferred() {
    if (!defer_upload || finished) return MH_OK;
    MH_TRY(set_device(ctx));
    MH_HIP(hipMemcpyAsync(ctx->sched.p, ctx->h_sched.p, nsched_pending * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(hipMemcpyAsync(ctx->d_state, ctx->h_state, kParamsOffset + sizeof(IcpDeviceParams), hipMemcpyHostToDevice,
                          ctx->stream));
    defer_upload = false;
    return MH_OK;
  }

  // The whole loop in one launch, then the covariance kernels + the state read-back, one event wait.  Leaves `finished`
  // false when the loop did not run to its end (a workgroup gave up waiting for the others): the caller starts over with the
  // launch-by-launch chain.
  mh_status run_loop16() {
    MH_TRY(set_device(ctx));
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)scan->n;
    const uint32_t ngr = (n + kStepPoints - 1) / kStepPoints;
    const uint32_t max_steps = loop_steps, serial0 = loop_x.serial0;
    g_loop16_runs.fetch_add(1);
    void* const xa = loop_x.xa;
    void* const xb = loop_x.xb;
    const MapView mv = map->view(*sw);
    if (plan.loop == Loop::Icpw)
      hipLaunchKernelGGL(k_icpw, dim3((ngr + kLwGroups - 1) / kLwGroups), dim3(kLwThreads), 0, s, ctx->d_state, &ctx->d_params->mk,
                         &ctx->d_params->sk, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(),
                         xa, ngr, serial0, max_steps, p->compute_covariance ? 1u : 0u);
    else if (pl)
      hipLaunchKernelGGL(k_icp16<true>, dim3(ngr), dim3(kSolveThreads), 0, s, ctx->d_state, &ctx->d_params->mk, &ctx->d_params->sk, scan->x,
                         scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), ctx->pl_c.as<float4>(),
                         ctx->pl_n.as<float4>(), xa, xb, ngr, serial0, max_steps, p->compute_covariance ? 1u : 0u);
    else
      hipLaunchKernelGGL(k_icp16<false>, dim3(ngr), dim3(kSolveThreads), 0, s, ctx->d_state, &ctx->d_params->mk, &ctx->d_params->sk, scan->x,
                         scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), (float4*)nullptr,
                         (float4*)nullptr, xa, xb, ngr, serial0, max_steps, p->compute_covariance ? 1u : 0u);
    enqueued = p->max_iterations;
    skip_tail = false;
    MH_TRY(enqueue_tail(/*cov_prepared=*/true));
    const hipError_t we = mh::wait_event(ctx->ev_poll);
    loop_adm.release();
    MH_HIP(we);
    const IcpDeviceState* h = ctx->h_state;
    if (!h->done || h->handover_timeouts) {
      g_loop16_fallbacks.fetch_add(1);
      if (!sw->loop16_test_abandon) loop_holdoff(ctx->device, 1);
      return MH_OK;  // (not finished)
    }
    loop_holdoff(ctx->device, -1);
    return poll(true);
  }

  mh_status enqueue_chunk() {
    if (finished) return MH_OK;
    MH_TRY(set_device(ctx));
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)scan->n;
    const MapView mv = map->view(*sw);
    const Matcher mt = plan.matcher;
    const uint32_t m = (p->max_iterations - enqueued) < chunk ? (p->max_iterations - enqueued) : chunk;
    PoseArg dummy{};
    double* part = ctx->partials.as<double>();
    const MatchK* dmk = &ctx->d_params->mk;
    const SolveK* dsk = &ctx->d_params->sk;
    // everything a chunk launches, in stream order; used directly (profiling / MH_NO_GRAPH) or under stream capture
    const bool step_chain = plan.step_chain;  // k_step16: every launch over the whole layer, the solve carried into the next launch
    const uint32_t ngr = n ? (n + kStepPoints - 1) / kStepPoints : 1u;
    const uint32_t nwg = ngr < kStepMaxWorkgroups ? ngr : kStepMaxWorkgroups;
    // (launches whose arguments may be frozen in a captured graph cannot be told their number)
    const bool counted = prof || streaming || sw->no_graph;
    uint32_t chunk_k = 0;  // k_step16 launches of this chunk so far
    auto launch_step = [&](uint32_t close_only) {
      const uint32_t expect = counted ? serial_base + step_launches : chunk_k;  // (replayed: the place in the chunk)
      const uint32_t expect_rel = counted ? 0u : 1u;
      step_launches++;
      chunk_k++;
      // canonical block (upload, results) + a ping-pong pair: a launch never writes the block it reads, and the canonical one is only
      // written by launches that do not read it (the one that ends the loop, the one-workgroup close-only launch)
      IcpDeviceState* const S[3] = {ctx->d_state_b, reinterpret_cast<IcpDeviceState*>(reinterpret_cast<char*>(ctx->d_state_b) + 256), ctx->d_state};
      const uint32_t src = step_src, dst = close_only ? 2u : (src == 2u ? 0u : (src ^ 1u));
      double* const pa[2] = {part, part + (size_t)kStepRowsA * ngr};
      double* const pbb = pl ? ctx->partials_b.as<double>() : nullptr;
      double* const pb[2] = {pbb, pbb ? pbb + (size_t)kStepRowsB * ngr : nullptr};
      const uint32_t par = step_ppar;
      if (pl)
        hipLaunchKernelGGL(k_step16<true>, dim3(close_only ? 1u : nwg), dim3(kSolveThreads), 0, s, S[src], S[dst],
                           S[2], dmk, dsk, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(),
                           ctx->pl_c.as<float4>(), ctx->pl_n.as<float4>(), (const double*)pa[par], pa[par ^ 1u], (const double*)pb[par],
                           pb[par ^ 1u], ngr, close_only, expect, expect_rel);
      else
        hipLaunchKernelGGL(k_step16<false>, dim3(close_only ? 1u : nwg), dim3(kSolveThreads), 0, s, S[src], S[dst],
                           S[2], dmk, dsk, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(),
                           (float4*)nullptr, (float4*)nullptr, (const double*)pa[par], pa[par ^ 1u], (const double*)nullptr,
                           (double*)nullptr, ngr, close_only, expect, expect_rel);
      step_src = dst;
      if (!close_only) step_ppar = par ^ 1u;
    };
    auto enqueue_kernels = [&]() -> mh_status {
      double* partb = pl ? ctx->partials_b.as<double>() : nullptr;
      const bool rows16 = pl && mt == Matcher::Row;              // NDT layer handled by the row kernel
      const uint32_t nB = pl ? (rows16 ? nba : nb) : 0u;       // columns of the point-to-plane partials of the FIRST step
      const uint32_t nBi = pl ? nba : 0u;                      // ... of the inner steps (k_accum_both)
      for (uint32_t j = 0; j < m; j++) {
        if (step_chain) {
          for (uint32_t in = 0; in < p->gn.max_inner_iterations; in++) launch_step(0u);
          continue;
        }
        const bool both16 = pl && mt == Matcher::Row;  // small layer: both matchers in one launch (k_match16<true>)
        if (pl && !both16)
          hipLaunchKernelGGL(k_match_pl<true>, dim3(nb), dim3(kBlock), 0, s, ctx->d_state, dummy, 0.f, dmk, scan->x, scan->y,
                             scan->z, n, mv, ctx->pl_c.as<float4>(), ctx->pl_n.as<float4>(), partb, nb);
        if (prof) MH_HIP(hipEventRecord(ctx->prof_ev[2 * prof_n], s));
        if (mt == Matcher::Row) {
          if (plan.fused16)
            hipLaunchKernelGGL((k_match16<false, true>), dim3(nbm), dim3(kBlock), 0, s, ctx->d_state, dmk, scan->x, scan->y,
                               scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), (float4*)nullptr,
                               (float4*)nullptr, part, nbm);
          else if (both16)
            hipLaunchKernelGGL((k_match16<true, false>), dim3((uint32_t)((16ull * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ctx->d_state,
                               dmk, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(),
                               ctx->pl_c.as<float4>(), ctx->pl_n.as<float4>(), (double*)nullptr, 0u);
          else
            hipLaunchKernelGGL((k_match16<false, false>), dim3((uint32_t)((16ull * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ctx->d_state,
                               dmk, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(),
                               (float4*)nullptr, (float4*)nullptr, (double*)nullptr, 0u);
          if (prof) MH_HIP(hipEventRecord(ctx->prof_ev[2 * prof_n + 1], s));  // the match kernel alone
          if (both16)  // both kinds of Gauss-Newton rows of the pairings just written
            hipLaunchKernelGGL(k_accum_both, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 1u, dmk, scan->x, scan->y, scan->z, n,
                               ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), ctx->pl_c.as<float4>(),
                               ctx->pl_n.as<float4>(), part, partb, nba);
          else if (!plan.fused16)
            hipLaunchKernelGGL(k_accum<false>, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 1u, dmk, scan->x, scan->y, scan->z, n,
                               ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nbm);
        } else if (mt == Matcher::Flat) {
          hipLaunchKernelGGL(flat32 ? k_match_flat<true> : k_match_flat<false>, dim3(nblk_flat(n)), dim3(kFlatThreads), 0, s,
                             ctx->d_state, scan->x, scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>());
          ctx->flat_issued[flat32 ? 0 : 1]++;  // (enqueue_cached counts them: now, or whenever the captured chunk is launched)
          if (prof) MH_HIP(hipEventRecord(ctx->prof_ev[2 * prof_n + 1], s));  // the match kernel alone
          hipLaunchKernelGGL(k_accum<true>, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 1u, dmk, scan->x, scan->y, scan->z, n,
                             ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nba);
        } else if (mt == Matcher::Quad) {
          hipLaunchKernelGGL(k_match4, dim3((uint32_t)((4ull * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ctx->d_state, scan->x, scan->y,
                             scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>());
          if (prof) MH_HIP(hipEventRecord(ctx->prof_ev[2 * prof_n + 1], s));  // the match kernel alone
          hipLaunchKernelGGL(k_accum<false>, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 1u, dmk, scan->x, scan->y, scan->z, n,
                             ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nba);
        } else if (mt == Matcher::Literal)
          hipLaunchKernelGGL((k_match<true, 0>), dim3(nb), dim3(kBlock), 0, s, ctx->d_state, dummy, 0.f, 1u, dmk, scan->x,
                             scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nbm);
        else
          hipLaunchKernelGGL((k_match<true, 1>), dim3(nb), dim3(kBlock), 0, s, ctx->d_state, dummy, 0.f, 1u, dmk, scan->x,
                             scan->y, scan->z, n, mv, ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nbm);
        if (prof) {
          if (one_lane(mt)) MH_HIP(hipEventRecord(ctx->prof_ev[2 * prof_n + 1], s));
          prof_n++;
        }
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, dsk, part, nbm, nbm,
                           (const double*)partb, nB, nB, 1u);
        for (uint32_t in = 1; in < p->gn.max_inner_iterations; in++) {
          if (pl)
            hipLaunchKernelGGL(k_accum_both, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 0u, dmk, scan->x, scan->y, scan->z, n,
                               ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), ctx->pl_c.as<float4>(),
                               ctx->pl_n.as<float4>(), part, partb, nba);
          else
            hipLaunchKernelGGL(mt == Matcher::Flat ? k_accum<true> : k_accum<false>, dim3(nba), dim3(kBlock), 0, s, ctx->d_state, 0u, dmk, scan->x, scan->y, scan->z, n,
                               ctx->pair_q.as<float4>(), ctx->pair_gidx.as<uint32_t>(), part, nba);
          hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, dsk, part, nba, nba,
                             (const double*)partb, nBi, nBi, 0u);
        }
      }
      // the step chain's last Gauss-Newton step is still pending: at the end of a chunk the host is going to look at the state,
      // under streaming control only once the iteration budget is queued (a loop that ends earlier is seen by the next launch)
      if (step_chain && (!skip_tail || enqueued + m >= p->max_iterations)) launch_step(1u);
      if (skip_tail) return MH_OK;  // streaming: the tail below is enqueued once, by enqueue_tail()
      return enqueue_cov_and_state(false);
    };
    // (the launches of a streamed chunk follow the progress word, those of a profiled one carry events: never from a graph)
    const bool direct = prof || sw->no_graph || streaming;
    unsigned long long key[32] = {0};
    if (!direct) {
      if (step_chain) {  // the serial number this chunk's first k_step16 launch has to find (its launches carry their place in the chunk)
        ctx->h_params->sk.step_base = serial_base + step_total;
        MH_HIP(hipMemcpyAsync(&ctx->d_params->sk.step_base, &ctx->h_params->sk.step_base, sizeof(uint32_t), hipMemcpyHostToDevice, s));
        step_total += m * p->gn.max_inner_iterations + ((!skip_tail || enqueued + m >= p->max_iterations) ? 1u : 0u);
      }
      uint32_t fb;
      memcpy(&fb, &mv.inv_vs, 4);
      const unsigned long long kv[] = {n, nb, nbm, (unsigned long long)mt, m, p->gn.max_inner_iterations,
                                       p->compute_covariance, (unsigned long long)mv.slots, (unsigned long long)mv.pts, mv.mask,
                                       fb, mv.trunc | (mv.ndt << 1) | (mv.no_prev_bound << 2), (unsigned long long)scan->x, (unsigned long long)scan->y,
                                       (unsigned long long)scan->z, (unsigned long long)ctx->pair_q.p,
                                       (unsigned long long)ctx->pair_gidx.p, (unsigned long long)part,
                                       (unsigned long long)ctx->d_state, (unsigned long long)ctx->d_params,
                                       (unsigned long long)ctx->h_state,
                                       (pl ? 2ull : 1ull) | (plan.fused16 ? 8ull : 0ull) | (step_chain ? 16ull : 0ull) | (flat32 ? 32ull : 0ull),
                                       (unsigned long long)(pl ? ctx->pl_c.p : nullptr),
                                       (unsigned long long)(pl ? ctx->pl_n.p : nullptr),
                                       (unsigned long long)(pl ? ctx->partials_b.p : nullptr),
                                       (unsigned long long)mv.pts_q};  // (a word each: no XOR folding)
      static_assert(sizeof(kv) <= sizeof(key), "graph key too small");
      memcpy(key, kv, sizeof(kv));
    }
    MH_TRY(enqueue_cached(ctx, direct, key, enqueue_kernels));
    enqueued += m;
    if (streaming) return MH_OK;  // (no event per iteration: the progress word is the signal)
    if (prof) MH_HIP(hipEventRecord(ctx->ev_t1, s));
    MH_HIP(hipEventRecord(ctx->ev_poll, s));
    return MH_OK;
  }

  // The whole loop of a single alignment under streaming control: iterations are enqueued one at a time, at most `lead`
  // ahead of the iteration the device has published; once it publishes "done" the covariance kernels and the state
  // read-back follow and ONE event wait ends the call.
  mh_status run_streaming() {
    const uint32_t lead = kStreamLead + (plan.step_chain ? 1u : 0u);  // (k_step16 publishes an iteration's end from the NEXT launch)
    volatile uint32_t* prog = ctx->h_progress;
    *prog = 0;  // (the previous alignment of this context has been waited for: nothing in flight writes it)
    chunk = 1;
    skip_tail = true;
    uint32_t spins = 0;
    for (;;) {
      const uint32_t pv = *prog;
      if (pv >> 31) break;
      const uint32_t dev_iter = pv & 0x7FFFFFFFu;
      if (enqueued < p->max_iterations && enqueued < dev_iter + lead) {
        MH_TRY(enqueue_chunk());
        spins = 0;
        continue;
      }
      __builtin_ia32_pause();
      if (++spins > (1u << 22)) {  // ~ tens of milliseconds without progress: is the stream still alive?
        spins = 0;
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return fail(MH_ERR_HIP, "device ICP loop: %s", hipGetErrorString(q));
        if (q == hipSuccess && !(*prog >> 31) && enqueued >= p->max_iterations)
          return fail(MH_ERR_INTERNAL, "device ICP loop did not terminate after max_iterations");
      }
    }
    skip_tail = false;
    chunk = 0;
    MH_TRY(enqueue_tail());  // the tail alone: covariance (now live: the loop has ended) + state read-back
    return poll();
  }

  // the covariance kernels (no-ops unless the loop has terminated; cov_prepared: k_icp16 has done k_cov_prepare's part) and the
  // state read-back: what ends every chunk the host is going to look at
  mh_status enqueue_cov_and_state(bool cov_prepared) {
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)scan->n;
    double* part = ctx->partials.as<double>();
    double* partb = pl ? ctx->partials_b.as<double>() : nullptr;
    if (p->compute_covariance) {
      if (!cov_prepared) hipLaunchKernelGGL(k_cov_prepare, dim3(1), dim3(64), 0, s, ctx->d_state, &ctx->d_params->sk, 0u);
      hipLaunchKernelGGL(k_cov_accum, dim3(nb), dim3(kBlock), 0, s, ctx->d_state, 0u, scan->x, scan->y, scan->z, n,
                         ctx->pair_gidx.as<uint32_t>(), part, nb);
      if (pl)
        hipLaunchKernelGGL(k_cov_accum_plbuf, dim3(nb), dim3(kBlock), 0, s, ctx->d_state, scan->x, scan->y, scan->z, n,
                           ctx->pl_c.as<float4>(), ctx->pl_n.as<float4>(), partb, nb);
      hipLaunchKernelGGL(k_cov_finalize, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, 0u, part, nb, nb,
                         (const double*)partb, pl ? nb : 0u, pl ? nb : 0u);  // (the covariance kernels write nb columns)
    }
    MH_HIP(hipMemcpyAsync(ctx->h_state, ctx->d_state, sizeof(IcpDeviceState), hipMemcpyDeviceToHost, s));
    return MH_OK;
  }

  mh_status enqueue_tail(bool cov_prepared = false) {
    MH_TRY(set_device(ctx));
    MH_TRY(enqueue_cov_and_state(cov_prepared));
    MH_HIP(hipGetLastError());
    MH_HIP(hipEventRecord(ctx->ev_poll, ctx->stream));
    return MH_OK;
  }

  // waits for the last enqueued chunk; sets finished when the device loop has terminated
  mh_status poll(bool already_synced = false) {  // (lock-step batches copy the state into h_state themselves)
    if (finished) return MH_OK;
    polls++;
    MH_TRY(set_device(ctx));
    if (!already_synced) MH_HIP(mh::wait_event(ctx->ev_poll));
    const IcpDeviceState* h = ctx->h_state;
    if (!h->done && enqueued < p->max_iterations) {
      if (auto_chunk) chunk = kChunkNext;
      return MH_OK;
    }
    if (h->handover_timeouts)
      return fail(MH_ERR_INTERNAL, "device ICP loop (k_step16): %u workgroup(s) gave up waiting for the state block or the partial sums of the previous launch [first: kind %u wg %u tid %u wanted %u (base %u) seen %u groups %u expect %u state(pending|iter|inner|done) %08x iter %u n %u streaming %d]",
                  h->handover_timeouts, h->dbg[0], h->dbg[1], h->dbg[2], h->dbg[3], serial_base, h->dbg[4], h->dbg[5], h->dbg[6], h->dbg[7], h->n_iterations, (uint32_t)scan->n, (int)streaming);
    if (!h->done) return fail(MH_ERR_INTERNAL, "device ICP loop did not terminate after max_iterations");
    finished = true;
    if (auto_chunk) ctx->predicted_iterations[kind] = live_iterations(h);
    read_result(h, p, res, potential(), pl ? h->n_pairs_pl : 0u, polls, enqueued);
    if (trace) MH_TRY(download_trace(ctx, h, p, trace));
    if (prof) {
      float ms = 0.f;
      double sum = 0.0;
      // launches enqueued after termination are early-exit no-ops; time only the live ones
      uint32_t live = live_iterations(h);
      if (live > prof_n) live = prof_n;
      for (uint32_t i = 0; i < live; i++) {
        MH_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        sum += ms;
      }
      res->n_match_launches = live;
      res->match_kernel_ms = sum;
      MH_HIP(hipEventElapsedTime(&ms, ctx->ev_t0, ctx->ev_t1));
      res->total_ms = ms;
    }
    return MH_OK;
  }
};

mh_status check_align_args(const mh_map* map, const mh_scan* scan, const mh_icp_params* p, const double* T,
                           const mh_icp_result* res) {
  MH_REQUIRE(map && scan && p && T && res, "null argument");
  MH_REQUIRE(map->ctx->device == scan->ctx->device, "map and scan live on different devices");
  MH_REQUIRE(pose_ok(T), "non-finite initial guess");
  MH_REQUIRE(p->max_iterations == 0 || (p->threshold && p->kernel_param), "threshold/kernel_param arrays are required");
  MH_REQUIRE(p->gn.max_inner_iterations >= 1, "gn.max_inner_iterations must be >= 1");
  MH_REQUIRE(p->gn.robust_kernel <= MH_KERNEL_GM_C2, "unknown robust kernel");
  MH_REQUIRE(p->max_iterations < (1u << 20), "max_iterations too large");
  MH_REQUIRE(p->matched_points <= MH_MATCHED_POINTS_SKIP, "unknown matched_points mode");
  return MH_OK;
}

// mh_icp_align once its arguments are checked
mh_status align_single(const Switches& sw, const mh_map* map, const mh_scan* scan, const mh_icp_params* params,
                       const double T_guess[12], const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace,
                       const mh_pairs_out* final_pairs, int32_t pairs_mem) {
  AlignJob job;
  MH_TRY(job.start(sw, map, scan, params, T_guess, prior, result, trace));
  if (job.loop16 && !job.finished) {
    MH_TRY(job.run_loop16());
    if (!job.finished) {  // the loop's workgroups did not all get to run together: once more, launch by launch
      job.forbid_loop16 = true;
      MH_TRY(job.start(sw, map, scan, params, T_guess, prior, result, trace));
    }
  }
  if (job.streaming && !job.finished) MH_TRY(job.run_streaming());
  while (!job.finished) {
    MH_TRY(job.enqueue_chunk());
    MH_TRY(job.poll());
  }
  if (final_pairs && !job.trivial && result->n_final_pairs > result->n_final_pairs_pt2pl) {
    uint64_t np = 0;
    MH_TRY(compact_pairs(scan->ctx, scan->n, final_pairs, pairs_mem, &np));
    if (np != result->n_final_pairs - result->n_final_pairs_pt2pl)
      return fail(MH_ERR_INTERNAL, "pair compaction count mismatch: %llu pairings in the buffers, %u in the last accumulation",
                  (unsigned long long)np, result->n_final_pairs - result->n_final_pairs_pt2pl);
  }
  return MH_OK;
}

#include "mh_icp_layers.inl"  // LayersView, check_layers_job, LayersJob, align_layers_as (mh_icp_align_layers*)

}  // namespace

extern "C" {

mh_status mh_icp_align(const mh_map* map, const mh_scan* scan, const mh_icp_params* params, const double T_guess[12],
                       const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace, const mh_pairs_out* final_pairs,
                       int32_t pairs_mem) {
  MH_TRY(check_align_args(map, scan, params, T_guess, result));
  MH_REQUIRE(!final_pairs || pairs_mem == MH_MEM_HOST || pairs_mem == MH_MEM_DEVICE, "bad mem space");
  return align_single(read_switches(), map, scan, params, T_guess, prior, result, trace, final_pairs, pairs_mem);
}

mh_status mh_icp_align_prefers_solo(const mh_scan* scan, const mh_icp_params* p, uint32_t concurrent_callers, int32_t* yes) {
  MH_REQUIRE(scan && p && yes, "null argument");
  // what AlignJob::start decides for a single alignment under automatic control: a one-launch loop ...
  const Switches sw = read_switches();
  const AlignPlan a = plan_alignment(sw, scan->n, p->pt2pl_threshold != nullptr, p->matched_points, nullptr, p->profile != 0,
                                     p->poll_every == 0 && scan->ctx->d_progress != nullptr);
  // ... and the loops of all callers fit the device together: nobody waits for a turn.  (70 % of the CUs: the callers' filters,
  // de-skew and map updates run beside the loops -- five loops of 44 workgroups on 256 CUs measured slower than four, 3780 against
  // 4000-4450 scans/s.)
  *yes = (p->max_iterations > 0 && a.loop != Loop::None && a.loop_units &&
          loops_fit(sw, scan->ctx->device, a.loop_units, concurrent_callers)) ? 1 : 0;
  return MH_OK;
}

int32_t mh_debug_dev_variants(void) {
  return 0;
}

void mh_debug_loop_stats(uint64_t* loops_started, uint64_t* loops_abandoned) {
  if (loops_started) *loops_started = g_loop16_runs.load();
  if (loops_abandoned) *loops_abandoned = g_loop16_fallbacks.load();
}

void mh_debug_flat_stats(uint64_t launches[4]) {
  if (!launches) return;
  for (int k = 0; k < 4; k++) launches[k] = g_flat_launches[k].load(std::memory_order_relaxed);
}

size_t mh_pairs_block_bytes(size_t n_scan_points) {
  const size_t S = ((n_scan_points ? n_scan_points : 1) + 63) / 64 * 64;
  return 6 * S * sizeof(uint32_t);
}

#include "mh_icp_batch.inl"  // mh_icp_align_batch

#include "mh_icp_api.inl"    // mh_nn_search*, mh_gn_solve, mh_covariance

// Five spellings of one call: each fills the job description (mh_layer_job_planes) and takes the shared path, align_layers_as.
mh_status mh_icp_align_layers_planes(size_t n_pairs, const mh_layer_pair* pairs, const mh_layer_pair_opts* opts,
                                     const mh_layer_pair_gates* gates, const mh_layer_pair_knn* knn,
                                     const mh_layer_pair_plane* planes, const mh_icp_params* params, const double T_guess[12],
                                     const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace,
                                     const mh_pairs_out* final_pairs, const mh_pairs_pl_out* final_plane_pairs,
                                     uint64_t* final_pair_counts, int32_t pairs_mem) {
  return align_layers_as(__func__, {n_pairs, pairs, opts, gates, knn, planes}, params, T_guess, prior, result, trace, final_pairs,
                         final_plane_pairs, final_pair_counts, pairs_mem);
}

mh_status mh_icp_align_layers_kbest(size_t n_pairs, const mh_layer_pair* pairs, const mh_layer_pair_opts* opts,
                                    const mh_layer_pair_gates* gates, const mh_layer_pair_knn* knn, const mh_icp_params* params,
                                    const double T_guess[12], const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace,
                                    const mh_pairs_out* final_pairs, uint64_t* final_pair_counts, int32_t pairs_mem) {
  return align_layers_as(__func__, {n_pairs, pairs, opts, gates, knn, nullptr}, params, T_guess, prior, result, trace, final_pairs,
                         nullptr, final_pair_counts, pairs_mem);
}

mh_status mh_icp_align_layers_gated(size_t n_pairs, const mh_layer_pair* pairs, const mh_layer_pair_opts* opts,
                                    const mh_layer_pair_gates* gates, const mh_icp_params* params, const double T_guess[12],
                                    const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace,
                                    const mh_pairs_out* final_pairs, uint64_t* final_pair_counts, int32_t pairs_mem) {
  return align_layers_as(__func__, {n_pairs, pairs, opts, gates, nullptr, nullptr}, params, T_guess, prior, result, trace,
                         final_pairs, nullptr, final_pair_counts, pairs_mem);
}

mh_status mh_icp_align_layers_opts(size_t n_pairs, const mh_layer_pair* pairs, const mh_layer_pair_opts* opts,
                                   const mh_icp_params* params, const double T_guess[12], const mh_prior* prior,
                                   mh_icp_result* result, mh_icp_iter* trace, const mh_pairs_out* final_pairs,
                                   uint64_t* final_pair_counts, int32_t pairs_mem) {
  return align_layers_as(__func__, {n_pairs, pairs, opts, nullptr, nullptr, nullptr}, params, T_guess, prior, result, trace,
                         final_pairs, nullptr, final_pair_counts, pairs_mem);
}

mh_status mh_icp_align_layers(size_t n_pairs, const mh_layer_pair* pairs, const mh_icp_params* params, const double T_guess[12],
                              const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace, const mh_pairs_out* final_pairs,
                              uint64_t* final_pair_counts, int32_t pairs_mem) {
  return align_layers_as(__func__, {n_pairs, pairs, nullptr, nullptr, nullptr, nullptr}, params, T_guess, prior, result, trace,
                         final_pairs, nullptr, final_pair_counts, pairs_mem);
}

#include "mh_icp_layers_batch.inl"  // mh_icp_align_layers_batch

}  // extern "C"
