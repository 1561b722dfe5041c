// mh_k_match_kbest.h -- Matcher_Points_DistanceThreshold::pairingsPerPoint = k > 1 inside the multi-layer loop
// (mh_icp_align_layers_kbest; lidar2d.yaml:156, rgbd.yaml:138 use 2): the matcher of mh_nn_search_k -- per local point the k smallest
// (d2, scan position) of the 27-voxel block, accepted in that order while they pass the distance test -- as a bounded,
// wave-cooperative search, and the entry points of the loop's other kernels for a table that holds such a pair.
//
// Pairing segment of a pair with k > 1: point-major, entry e = i * k + r is the (r + 1)-th nearest record of local point i
// (k_match_kbest's layout: the compaction serves unchanged, local = e / k).  Conventions of match_flat_wave: the sign of .w is the
// verdict, |w| = inf means "no record at this rank", a rejected or missing entry has pair_gidx = kNoMatch.
//
// Search: the plan / scan matcher (mh_nn_flat.h, phases A1 / A2 / B) with K result words per point instead of one.  Phase B inserts
// a key with the RETURNING LDS minimum, slot by slot:  old = min-exchange(slot r, key); key = max(old, key); on to slot r + 1 until
// the key is the empty sentinel.  A slot keeps the smallest key it has ever been offered and hands every other one on exactly
// once, so slot r ends with the (r + 1)-th smallest key of the point whatever the order of arrival: integer minima only, bitwise
// reproducible, no lane holds a sorted list.  Keys (d2 bits << 32 | record position) are unique per record.
// Bound: from a pair's second active iteration on, b0 = the LARGEST d2 of the point's k previous partners under the new pose, when
// all k slots held a record (else the point has no bound).  Candidate voxels and quadrant narrowing use b0 as for k = 1; records with
// d2 <= b0 are inserted.  The tested records contain every record of the block within b0, so when slot k - 1 got filled the k
// smallest of the tested records are the block's (every untested record is farther than b0, hence farther than all k: no tie).  When
// it stayed empty a previous partner has left the block: the point is searched once more without a bound.
// What the plan does not cover -- points without a bound (a pair's first active iteration, MH_NO_PREV_BOUND=1: all of them; no
// own-voxel stage for them: NOT measured), more than kFlatMaxCand candidate voxels, chunk space exhausted, bound not attained --
// runs nn_search_kbest's scan, one lane per point, with an optional starting bound (nn_search_kbest_from).  The slow lanes search
// where they are: compacting them (phase D of match_flat_wave serves quads of lanes) saves nothing for one lane per point.
//
// Launches: pairs with k > 1 own no workgroup of k_match_layers; k_match_layers_k walks a flattened block range over them only
// (KnnTable, as k_claim_layers walks the unique pairs) and is enqueued only when such a pair exists.  The accumulation and the
// covariance of such a table are k_accum_layers_k / k_cov_accum_layers_k INSTEAD of k_accum_layers / k_cov_accum_layers: the same
// bodies over n * k entries with the local point e / k (a pair with k = 1 divides by one: its columns keep their bits), so the
// kernels of a table without such a pair stay the code objects they were.
#pragma once

namespace mh {

// KS result slots per point on top of a plan / scan wave BASE (the k-best pairs: kMaxKnn slots on FlatWave; the plane search of
// mh_k_match_planes.h widens both through these parameters, so the kernels here keep their code objects and their LDS footprint)
template <int KS, class BASE = FlatWave>
struct FlatWaveKT : BASE {
  unsigned long long RESK[KS * 64];  // slot r of point p: RESK[r * 64 + p] (the wave's points side by side: no bank conflicts)
};
typedef FlatWaveKT<kMaxKnn> FlatWaveK;

template <int KS>
struct FlatInsertKT {
  uint32_t k;
  template <class FW>
  __device__ __forceinline__ void operator()(FW& sh, uint32_t p, unsigned long long key) const {
    // (a fixed trip count under predicates: phase B's loop over its records in flight stays unrolled, its arrays in registers)
#pragma unroll
    for (int r = 0; r < KS; r++) {
      if ((uint32_t)r < k && key != ~0ull) {  // (~0: the slot's initial value has moved on -- nothing left to place)
        const unsigned long long old =
            __hip_atomic_fetch_min(&sh.RESK[(uint32_t)r * 64u + p], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        key = old > key ? old : key;  // the smaller one stays, the larger moves on
      }
    }
  }
};
typedef FlatInsertKT<kMaxKnn> FlatInsertK;

// nn_search_kbest (mh_nn_device.h) with a starting bound b0 (+inf: none, and then the same search): only records with d2 <= b0
// are kept, voxels are pruned against b0 until k records are found and against the k-th smallest from then on.  best[] ascending
// on return, entries never filled stay ~0; with a bound the result is the block's iff best[k - 1] got filled.
__device__ __forceinline__ void knn_visit_within(const MapView& m, gslots_ptr slots4, gpts_ptr pts4, unsigned long long key, float qx,
                                                 float qy, float qz, float b0, knnkey_t (&best)[kMaxKnn]) {
  uint32_t h = hash_key(key) & m.mask;
  u32x4 sl = slots4[h];
  unsigned long long sk = ((unsigned long long)sl.y << 32) | sl.x;
  while (sk != key && sk != kEmptyKey) {  // linear probing past a collision
    h = (h + 1) & m.mask;
    sl = slots4[h];
    sk = ((unsigned long long)sl.y << 32) | sl.x;
  }
  if (sk != key) return;
  const uint32_t n_rec = slot_count(sl.w);
  for (uint32_t j = 0; j < n_rec; j++) {
    const f32x4 c = pts4[sl.z + j];
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;  // fp32, un-fused, this order (bit-exact with the oracle)
    if (!(d2 > b0)) knn_insert<kMaxKnn>(best, ((knnkey_t)__float_as_uint(d2) << 32) | (knnkey_t)(sl.z + j));
  }
}
// best[k - 1] of an ascending list as the maximum of its first k entries (~0 while one of them is unfilled): arithmetic on the
// values, which keeps best[] in registers where a chain of selects on the index became an indexed load from scratch here
__device__ __forceinline__ knnkey_t knn_kth(const knnkey_t (&best)[kMaxKnn], uint32_t k) {
  knnkey_t v = 0;
#pragma unroll
  for (int t = 0; t < kMaxKnn; t++) {
    const knnkey_t b = (uint32_t)t < k ? best[t] : 0ull;
    v = b > v ? b : v;
  }
  return v;
}
__device__ __forceinline__ void nn_search_kbest_from(const MapView& m, float qx, float qy, float qz, uint32_t k, float b0,
                                                     knnkey_t (&best)[kMaxKnn]) {
#pragma unroll
  for (int t = 0; t < kMaxKnn; t++) best[t] = ~0ull;
  const float lim = 1.0e6f;
  if (!((int)(fabsf(qx * m.inv_vs) < lim) & (int)(fabsf(qy * m.inv_vs) < lim) & (int)(fabsf(qz * m.inv_vs) < lim))) return;
  const int cx = voxel_of(qx, m.inv_vs, m.trunc), cy = voxel_of(qy, m.inv_vs, m.trunc), cz = voxel_of(qz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const Gaps gx = axis_gaps(qx, cx, m.vs, m.trunc), gy = axis_gaps(qy, cy, m.vs, m.trunc), gz = axis_gaps(qz, cz, m.vs, m.trunc);
  knn_visit_within(m, slots4, pts4, nn_key_of(kbase, 13), qx, qy, qz, b0, best);
#pragma unroll 1
  for (int c = 0; c < 27; c++) {
    if (c == 13) continue;
    // the k-th smallest distance so far, b0 while fewer than k were found (every kept record is within b0)
    const knnkey_t kth = knn_kth(best, k);
    const float bound = kth != ~0ull ? __uint_as_float((uint32_t)(kth >> 32)) : b0;
    if (nn_lower_bound(c, gx, gy, gz) * 0.9999f > bound) continue;
    knn_visit_within(m, slots4, pts4, nn_key_of(kbase, c), qx, qy, qz, b0, best);
  }
}

// One wave, 64 consecutive local points of a pair with k pairings per point, starting at `i0` (lanes past `n` idle).
__device__ __forceinline__ void match_kbest_wave(FlatWaveK& sh, const MapView& m, const double* __restrict__ T, float thr2, float ang2,
                                                 bool have_prev, const float* __restrict__ lx, const float* __restrict__ ly,
                                                 const float* __restrict__ lz, uint32_t n, uint32_t k, uint32_t i0,
                                                 float4* __restrict__ pair_q, uint32_t* __restrict__ pair_gidx) {
  const uint32_t lane = (uint32_t)__lane_id();
  const uint32_t i = i0 + lane;
  const bool in = i < n;
  const uint32_t ic = in ? i : n - 1;
  const size_t e0 = (size_t)ic * k;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const auto gq = G(reinterpret_cast<f32x4*>(pair_q));
  // ---- A1: the point --------------------------------------------------------------------------------------------------
  const float x = G(lx)[ic], y = G(ly)[ic], z = G(lz)[ic];
  float px, py, pz;
  transform_point(T, x, y, z, px, py, pz);
  float b0 = __builtin_inff();
  if (have_prev) {  // grid-uniform
    bool all = true;
    float far = 0.f;
    for (uint32_t r = 0; r < k; r++) {
      const f32x4 prev = gq[e0 + r];
      all = all && fabsf(prev.w) < __builtin_inff();  // (the sign is the verdict)
      const float dx = prev.x - px, dy = prev.y - py, dz = prev.z - pz;
      far = fmaxf(far, (dx * dx + dy * dy) + dz * dz);  // the candidate arithmetic
    }
    if (all) b0 = far;  // attained by k records
  }
  const float lim = 1.0e6f;
  const bool okrange = ((int)(fabsf(px * m.inv_vs) < lim) & (int)(fabsf(py * m.inv_vs) < lim) & (int)(fabsf(pz * m.inv_vs) < lim)) != 0;
  const int cx = voxel_of(px, m.inv_vs, m.trunc), cy = voxel_of(py, m.inv_vs, m.trunc), cz = voxel_of(pz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  bool planned = in && okrange && b0 < __builtin_inff();
  uint32_t cmask = 0;
  MH_FLATDBG(10, in);
  MH_FLATDBG(11, in && !planned);
  if (__ballot(planned) != 0ull) {  // wave-uniform
    // every voxel whose lower bound does not exceed b0 (match_flat_wave has the argument for the seven-test form)
    const Gaps gx = axis_gaps(px, cx, m.vs, m.trunc), gy = axis_gaps(py, cy, m.vs, m.trunc), gz = axis_gaps(pz, cz, m.vs, m.trunc);
    cmask = 1u << 13;
    const float fx = fmaxf(gx.s[0], gx.s[2]), fy = fmaxf(gy.s[0], gy.s[2]), fz = fmaxf(gz.s[0], gz.s[2]);
    const bool far_dead = (fx * 0.9999f > b0) && (fy * 0.9999f > b0) && (fz * 0.9999f > b0);
    if (__ballot(planned && !far_dead) == 0ull) {  // wave-uniform
      const bool xl = gx.s[0] <= gx.s[2], yl = gy.s[0] <= gy.s[2], zl = gz.s[0] <= gz.s[2];
      const float nx = xl ? gx.s[0] : gx.s[2], ny = yl ? gy.s[0] : gy.s[2], nz = zl ? gz.s[0] : gz.s[2];
      const uint32_t cx_ = xl ? 4u : 22u, cy_ = yl ? 10u : 16u, cz_ = zl ? 12u : 14u;  // 13 -/+ 9, 3, 1
      const uint32_t dx_ = cx_ - 13u, dy_ = cy_ - 13u;                               // (mod 2^32)
      const float lxy = nx + ny;
      cmask |= (!(nx * 0.9999f > b0)) ? (1u << cx_) : 0u;
      cmask |= (!(ny * 0.9999f > b0)) ? (1u << cy_) : 0u;
      cmask |= (!(nz * 0.9999f > b0)) ? (1u << cz_) : 0u;
      cmask |= (!(lxy * 0.9999f > b0)) ? (1u << (cy_ + dx_)) : 0u;
      cmask |= (!((nx + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_)) : 0u;
      cmask |= (!((ny + nz) * 0.9999f > b0)) ? (1u << (cz_ + dy_)) : 0u;
      cmask |= (!((lxy + nz) * 0.9999f > b0)) ? (1u << (cz_ + dx_ + dy_)) : 0u;
    } else {
#pragma unroll
      for (int c = 0; c < 27; c++) {
        if (c == 13) continue;
        const int ix = c / 9, iy = (c / 3) % 3, iz = c % 3;
        const float sx = ix == 1 ? 0.f : gx.s[ix], sy = iy == 1 ? 0.f : gy.s[iy], sz = iz == 1 ? 0.f : gz.s[iz];
        const float lb = ((sx + sy) + sz) * 0.9999f;  // quad_bounds' expression
        cmask |= (!(lb > b0)) ? (1u << c) : 0u;
      }
    }
    if (!planned) cmask = 0;
    MH_FLATDBG(12, __builtin_popcount(cmask) > kFlatMaxCand);
    if (__builtin_popcount(cmask) > kFlatMaxCand) {  // a loose bound near a voxel corner: the lane's own scan, with the bound
      planned = false;
      cmask = 0;
    }
    for (uint32_t r = 0; r < k; r++) sh.RESK[r * 64u + lane] = ~0ull;  // (flat_plan_scan synchronises before phase B)
  }
  // ---- A2, B: the candidate voxels, the records -----------------------------------------------------------------------
  const uint32_t n_cands = flat_plan_scan(sh, m, lane, cmask, kbase, px, py, pz, b0, ~0ull, FlatInsertK{k});
  // ---- C: the k smallest ------------------------------------------------------------------------------------------------
  knnkey_t best[kMaxKnn];
#pragma unroll
  for (int t = 0; t < kMaxKnn; t++) best[t] = ~0ull;
  bool slow = in && !planned;
  float b0s = b0;  // the bound the lane's own scan starts from
  if (planned) {   // (a planned lane has its own voxel among the candidates: n_cands > 0)
    const bool spilled = n_cands == 0u || sh.SLOWF[lane] != 0;
    if (!spilled && sh.RESK[(k - 1u) * 64u + lane] != ~0ull) {
#pragma unroll
      for (int t = 0; t < kMaxKnn; t++)
        if ((uint32_t)t < k) best[t] = sh.RESK[(uint32_t)t * 64u + lane];
    } else {
      slow = true;
      MH_FLATDBG(13, spilled);
      MH_FLATDBG(14, !spilled);
      if (!spilled) b0s = __builtin_inff();  // slot k - 1 stayed empty: a previous partner left the block -- once more, without the bound
    }
  }
  // ---- what the plan does not cover: one lane per point ---------------------------------------------------------------
  if (slow) {
    nn_search_kbest_from(m, px, py, pz, k, b0s, best);
    const bool again = b0s < __builtin_inff() && knn_kth(best, k) == ~0ull;
    MH_FLATDBG(15, again);
    if (again) nn_search_kbest_from(m, px, py, pz, k, __builtin_inff(), best);
  }
  if (!in) return;
  const float n2 = (px * px + py * py) + pz * pz;
  const float accept = thr2 + ang2 * n2;
#pragma unroll
  for (int t = 0; t < kMaxKnn; t++) {
    if ((uint32_t)t >= k) continue;  // (no break: the loop unrolls and best[] stays in registers)
    const knnkey_t key = best[t];
    const bool found = key != ~0ull;
    const float d2 = __uint_as_float((uint32_t)(key >> 32));
    f32x4 w = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (found) w = pts4[(uint32_t)key];
    const bool ok = found && d2 < accept;  // ascending distances against one limit: the accepted ones are a prefix
    gq[e0 + (uint32_t)t] = (f32x4){w.x, w.y, w.z, found ? flat_signed_d2(d2, ok) : -__builtin_inff()};
    G(pair_gidx)[e0 + (uint32_t)t] = ok ? __float_as_uint(w.w) : kNoMatch;
  }
}

}  // namespace mh

// the flattened block range of k_match_layers_k: pair i owns the workgroups [blk[i], blk[i + 1]) (a pair with k = 1: none)
struct KnnTable {
  uint32_t blk[MH_MAX_LAYER_PAIRS + 1];
  uint32_t pad;
};
typedef const KnnTable __attribute__((address_space(4))) * cknn_ptr;

// one wave of k_match_layers_k: workgroup `b` of the table's flattened k-best range (`cst`: the alignment's state, not terminated)
__device__ __forceinline__ void match_layers_k_wave(mh::FlatWaveK& sh, const clayers_state_ptr cst, const clayers_ptr ct,
                                                    const cknn_ptr ck, const uint32_t b) {
  const uint32_t li = layer_of(ck->blk, ct->n_pairs, b);
  const uint32_t n = ct->d[li].n, k = ct->d[li].kpp;
  const uint32_t i0 = (b - ck->blk[li]) * kFlatPointsPerBlock + (threadIdx.x & ~63u);
  if (i0 >= n) return;    // whole waves
  const uint32_t iter = cst->iter;
  if (!layer_active(ct, li, iter)) {  // (match_layers_wave: "not paired" for every entry of the pair, no bound left behind)
    const uint32_t i = i0 + (uint32_t)__lane_id();
    if (i < n)
      for (uint32_t r = 0; r < k; r++) {
        G(reinterpret_cast<f32x4*>(ct->d[li].pair_q))[(size_t)i * k + r] = (f32x4){0.f, 0.f, 0.f, -__builtin_inff()};
        G(ct->d[li].pair_gidx)[(size_t)i * k + r] = kNoMatch;
      }
    return;
  }
  MapView map;  // field by field: scalar loads through the constant-space table (match_layers_wave)
  map.slots = ct->d[li].map.slots;
  map.pts = ct->d[li].map.pts;
  map.mask = ct->d[li].map.mask;
  map.inv_vs = ct->d[li].map.inv_vs;
  map.vs = ct->d[li].map.vs;
  map.trunc = ct->d[li].map.trunc;
  map.ndt = ct->d[li].map.ndt;
  map.no_prev_bound = ct->d[li].map.no_prev_bound;
  map.pts_q = ct->d[li].map.pts_q;
  const bool have_prev = iter > ct->d[li].run_from && !map.no_prev_bound;
  double T[12];
#pragma unroll
  for (int j = 0; j < 12; j++) T[j] = cst->T[j];
  const double thr = G(ct->d[li].mk.thr)[iter];
  match_kbest_wave(sh, map, T, (float)(thr * thr), ct->d[li].mk.ang2, have_prev, ct->d[li].lx, ct->d[li].ly,
                   ct->d[li].lz, n, k, i0, ct->d[li].pair_q, ct->d[li].pair_gidx);
}

__global__ __launch_bounds__(kFlatThreads) void k_match_layers_k(const IcpDeviceState* __restrict__ st,
                                                                 const LayerTable* __restrict__ tab,
                                                                 const KnnTable* __restrict__ knn) {
  __shared__ FlatWaveK shk[kFlatThreads / 64];
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  match_layers_k_wave(shk[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(tab), (cknn_ptr)uniform_const_ptr(knn), blockIdx.x);
}

// k_match_layers_k for a lock-step group (mh_icp_align_layers_batch_opts, LayerBatchOptTable: mh_k_claim.h): the job by layer_of
// over the jobs' k-best prefix array, out when it has terminated, then the job's own KnnTable.  A job without a pair of k > 1 owns
// no workgroup here, a job whose pairs all have k > 1 none of k_match_layers_b.
__global__ __launch_bounds__(kFlatThreads) void k_match_layers_kb(const LayerBatchTable* __restrict__ bt,
                                                                  const LayerBatchOptTable* __restrict__ bo) {
  __shared__ FlatWaveK shk[kFlatThreads / 64];
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_opt_ptr co = (clayer_batch_opt_ptr)uniform_const_ptr(bo);
  const uint32_t ji = layer_of(co->job_blk_match_k, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  match_layers_k_wave(shk[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab),
                      (cknn_ptr)uniform_const_ptr(co->j[ji].knn), blockIdx.x - co->job_blk_match_k[ji]);
}

// k_accum_layers / k_cov_accum_layers for a table with a pair of k > 1: blk_acc / blk_cov are sized by the entries
__global__ __launch_bounds__(kBlock, MH_ACCUM_WAVES) void k_accum_layers_k(const IcpDeviceState* __restrict__ st,
                                                                           const LayerTable* __restrict__ tab, uint32_t first,
                                                                           double* __restrict__ partials, uint32_t pstride) {
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t li = layer_of(ct->blk_acc, ct->n_pairs, blockIdx.x);
  const uint32_t k = ct->d[li].kpp ? ct->d[li].kpp : 1u;
  k_accum_body<true, true>(st, first, &tab->d[li].mk, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n * k, ct->d[li].pair_q,
                           ct->d[li].pair_gidx, partials + ct->d[li].col_off, pstride, blockIdx.x - ct->blk_acc[li], k);
}

__global__ __launch_bounds__(kBlock) void k_cov_accum_layers_k(const IcpDeviceState* __restrict__ st,
                                                               const LayerTable* __restrict__ tab, double* __restrict__ partials,
                                                               uint32_t pstride) {
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t li = layer_of(ct->blk_cov, ct->n_pairs, blockIdx.x);
  const uint32_t k = ct->d[li].kpp ? ct->d[li].kpp : 1u;
  k_cov_accum_body<true>(st, 0u, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n * k, ct->d[li].pair_gidx,
                         partials + ct->d[li].cov_off, pstride, blockIdx.x - ct->blk_cov[li], k);
}

// ... and for a lock-step group with such a table among its jobs' (k_accum_layers_b / k_cov_accum_layers_b with the entries and
// their k: a job whose table has no such pair divides by one and keeps its bits)
__global__ __launch_bounds__(kBlock, MH_ACCUM_WAVES) void k_accum_layers_kb(const LayerBatchTable* __restrict__ bt, uint32_t first) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const uint32_t ji = layer_of(cb->job_blk_acc, cb->n_jobs, blockIdx.x);
  const IcpDeviceState* const st = cb->j[ji].st;
  if (((clayers_state_ptr)uniform_const_ptr(st))->done) return;  // uniform over the job's workgroups
  const LayerTable* const tab = cb->j[ji].tab;
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t b = blockIdx.x - cb->job_blk_acc[ji];
  const uint32_t li = layer_of(ct->blk_acc, ct->n_pairs, b);
  const uint32_t k = ct->d[li].kpp ? ct->d[li].kpp : 1u;
  k_accum_body<true, true>(st, first, &tab->d[li].mk, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n * k, ct->d[li].pair_q,
                           ct->d[li].pair_gidx, cb->j[ji].part + ct->d[li].col_off, cb->j[ji].tot_acc, b - ct->blk_acc[li], k);
}

__global__ __launch_bounds__(kBlock) void k_cov_accum_layers_kb(const LayerBatchTable* __restrict__ bt) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const uint32_t ji = layer_of(cb->job_blk_cov, cb->n_jobs, blockIdx.x);
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(cb->j[ji].tab);
  const uint32_t b = blockIdx.x - cb->job_blk_cov[ji];
  const uint32_t li = layer_of(ct->blk_cov, ct->n_pairs, b);
  const uint32_t k = ct->d[li].kpp ? ct->d[li].kpp : 1u;
  k_cov_accum_body<true>(cb->j[ji].st, 0u, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n * k, ct->d[li].pair_gidx,
                         cb->j[ji].part + ct->d[li].cov_off, cb->j[ji].tot_cov, b - ct->blk_cov[li], k);
}
