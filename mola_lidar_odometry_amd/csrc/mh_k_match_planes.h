// mh_k_match_planes.h -- Matcher_Point2Plane on a plain point layer (KNN + PCA; rgbd.yaml:143-151) inside the multi-layer loop
// (mh_icp_align_layers_planes): the matcher of mh_nn_search_pt2pl_knn as a bounded, wave-cooperative search with its result slots
// in LDS, and the entry points of the loop's other kernels for a table that holds such a pair.
//
// A plane pair's buffers: pl_c / pl_n, a float4 per local point, {centroid, 1 | 0} and {unit normal, 0} -- what acc_pt2pl_rows,
// k_cov_accum_plbuf_body and k_pl_flags / k_compact_pl read -- in the pair's own segment; its pair_q entry keeps what the next
// iteration's bound needs (below).  It owns no workgroup and no column of the plain kernels.
//
// Search: the plan / scan matcher (mh_nn_flat.h, phases A1 / A2 / B) with knn <= MH_MAX_PLANE_KNN result slots per point in LDS
// (FlatInsertKT: the returning-minimum chain of mh_k_match_kbest.h -- integer minima only, bitwise reproducible, no lane holds a
// sorted list) and up to 27 candidate voxels per point.
// The radius bound: the matcher only uses neighbours with d2 < searchRadius^2, so b0 = radius2 is a valid bound in EVERY
// iteration, the first included: the tested records contain every record of the block within it, the filled slots are the prefix
// of the block's knn nearest that the contract keeps, and fewer than knn found means there are no more inside the radius.  Phase
// B inserts d2 <= b0 while the contract is strict: the prefix test d2 < radius2 is applied afterwards, as k_match_pl_knn does.
// The previous-pairing bound: from a pair's second active iteration on, a point whose knn slots were all filled last time has
// left behind p'_prev and the distance d_k of its farthest partner.  Those knn records lie within d_k + |p' - p'_prev| of the
// new p' (triangle inequality), so the square of that -- when below radius2 -- bounds the search; it counts only when slot
// knn - 1 got filled (a previous partner can leave the 27-voxel block, and the rounding of the bound is not argued about), else
// the point is searched again under the radius bound.  MH_NO_PREV_BOUND=1 switches the tightening off; results do not depend on it.
// Chunk space: a wave's points under the radius bound can need more chunks than its LDS holds.  The points that did not fit are
// planned again on their own, pass after pass (each pass serves at least one point, or the rest goes one lane per point); the
// lane's own scan inserts into the same LDS slots -- there is no register list anywhere.
// PCA: the point's lane reads its slots back and calls pl_knn_plane (mh_k_match.h), the operation sequence of k_match_pl_knn.
//
// Launches: k_match_layers_pl walks a flattened range over the plane pairs only (PlaneTable) and is enqueued only when one
// exists; k_accum_layers_pl writes their Gauss-Newton rows into columns of the SECOND partials block that k_solve sums in fixed
// order behind the first, k_cov_accum_layers_pl likewise for the covariance.  The plain kernels stay the code objects they are.
// Lock-step batches (mh_icp_align_layers_batch_planes): the three bodies are __device__ functions that the *_pl_b entry points at
// the end of this file call too, one level up (job -> pair); k_solve_pl_b / k_cov_finalize_pl_b sum each job's two blocks.
#pragma once

namespace mh {

constexpr int kPlaneMaxChunks = 2048;
typedef FlatWaveKT<kMaxPlaneKnn, FlatWaveT<27, 64 * 27, kPlaneMaxChunks>> FlatWaveP;  // ~24 KB per wave
typedef FlatInsertKT<kMaxPlaneKnn> FlatInsertP;

// every voxel of the block whose lower bound does not exceed b0 (match_flat_wave has the argument for both forms); `lanes`:
// the lanes that plan in this pass (wave-uniform decisions are taken over them only)
__device__ __forceinline__ uint32_t plane_cand_mask(const MapView& m, bool lanes, float px, float py, float pz, int cx, int cy, int cz,
                                                    float b0) {
  const Gaps gx = axis_gaps(px, cx, m.vs, m.trunc), gy = axis_gaps(py, cy, m.vs, m.trunc), gz = axis_gaps(pz, cz, m.vs, m.trunc);
  uint32_t cmask = 1u << 13;
  const float fx = fmaxf(gx.s[0], gx.s[2]), fy = fmaxf(gy.s[0], gy.s[2]), fz = fmaxf(gz.s[0], gz.s[2]);
  const bool far_dead = (fx * 0.9999f > b0) && (fy * 0.9999f > b0) && (fz * 0.9999f > b0);
  if (__ballot(lanes && !far_dead) == 0ull) {  // wave-uniform
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
  return lanes ? cmask : 0u;
}

// the lane's own scan of the block: every record within b0 into the lane's LDS slots (voxels pruned against b0 only)
__device__ __forceinline__ void plane_scan_lane(FlatWaveP& sh, const MapView& m, uint32_t lane, float qx, float qy, float qz, int cx,
                                                int cy, int cz, float b0, const FlatInsertP ins) {
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  const gslots_ptr slots4 = (gslots_ptr)m.slots;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const Gaps gx = axis_gaps(qx, cx, m.vs, m.trunc), gy = axis_gaps(qy, cy, m.vs, m.trunc), gz = axis_gaps(qz, cz, m.vs, m.trunc);
#pragma unroll 1
  for (int c = 0; c < 27; c++) {
    if (c != 13 && nn_lower_bound(c, gx, gy, gz) * 0.9999f > b0) continue;
    const unsigned long long key = nn_key_of(kbase, c);
    uint32_t h = hash_key(key) & m.mask;
    u32x4 sl = slots4[h];
    unsigned long long sk = ((unsigned long long)sl.y << 32) | sl.x;
    while (sk != key && sk != kEmptyKey) {  // linear probing past a collision
      h = (h + 1) & m.mask;
      sl = slots4[h];
      sk = ((unsigned long long)sl.y << 32) | sl.x;
    }
    if (sk != key) continue;
    const uint32_t n_rec = slot_count(sl.w);
    for (uint32_t j = 0; j < n_rec; j++) {
      const f32x4 r = pts4[sl.z + j];
      const float dx = r.x - qx, dy = r.y - qy, dz = r.z - qz;
      const float d2 = (dx * dx + dy * dy) + dz * dz;  // fp32, un-fused, this order (bit-exact with the oracle)
      if (!(d2 > b0)) ins(sh, lane, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(sl.z + j));
    }
  }
}

// One wave, 64 consecutive local points of a plane pair starting at `i0` (lanes past `n` idle).  `a`: the matcher's parameters
// with this iteration's distance threshold.  prevq[i]: {p' of the point's last search, d_k or +inf} (read when have_prev, written
// always).
__device__ __forceinline__ void match_planes_wave(FlatWaveP& sh, const MapView& m, const double* __restrict__ T, const PlKnnArg& a,
                                                  bool have_prev, const float* __restrict__ lx, const float* __restrict__ ly,
                                                  const float* __restrict__ lz, uint32_t n, uint32_t i0, float4* __restrict__ prevq,
                                                  float4* __restrict__ pl_c, float4* __restrict__ pl_n) {
  const uint32_t lane = (uint32_t)__lane_id();
  const uint32_t i = i0 + lane;
  const bool in = i < n;
  const uint32_t ic = in ? i : n - 1;
  const uint32_t knn = a.knn;
  const gpts_ptr pts4 = (gpts_ptr)m.pts;
  const auto gprev = G(reinterpret_cast<f32x4*>(prevq));
  const FlatInsertP ins{knn};
  // ---- A1: the point ----------------------------------------------------------------------------------------------------
  const float x = G(lx)[ic], y = G(ly)[ic], z = G(lz)[ic];
  float px, py, pz;
  transform_point(T, x, y, z, px, py, pz);
  float bt = __builtin_inff();  // the tightened bound, when there is one below the radius bound
  if (have_prev) {              // grid-uniform
    const f32x4 prev = gprev[ic];
    if (prev.w < __builtin_inff()) {
      const float dx = prev.x - px, dy = prev.y - py, dz = prev.z - pz;
      const float reach = prev.w + sqrtf((dx * dx + dy * dy) + dz * dz);
      const float b = (reach * reach) * 1.0001f;
      if (b < a.radius2) bt = b;
    }
  }
  const float lim = 1.0e6f;
  const bool okrange = ((int)(fabsf(px * m.inv_vs) < lim) & (int)(fabsf(py * m.inv_vs) < lim) & (int)(fabsf(pz * m.inv_vs) < lim)) != 0;
  const int cx = voxel_of(px, m.inv_vs, m.trunc), cy = voxel_of(py, m.inv_vs, m.trunc), cz = voxel_of(pz, m.inv_vs, m.trunc);
  const unsigned long long kbase = pack_key(cx - 1, cy - 1, cz - 1);
  // ---- A2, B: pass after pass until every point of the wave has its slots ---------------------------------------------
  bool pending = in && okrange;  // (out of range: no record, as nn_search_kbest)
  bool tight_pass = __ballot(pending && bt < __builtin_inff()) != 0ull;  // wave-uniform
#pragma unroll 1
  while (__ballot(pending) != 0ull) {
    const bool act = pending && (!tight_pass || bt < __builtin_inff());
    const float b0 = tight_pass ? bt : a.radius2;
    const uint32_t cmask = plane_cand_mask(m, act, px, py, pz, cx, cy, cz, b0);
    if (act)
      for (uint32_t r = 0; r < knn; r++) sh.RESK[r * 64u + lane] = ~0ull;  // (flat_plan_scan synchronises before phase B)
    const uint32_t n_cands = flat_plan_scan(sh, m, lane, cmask, kbase, px, py, pz, b0, ~0ull, ins);
    // (an active lane has its own voxel among the candidates: n_cands > 0)
    const bool spilled = act && (n_cands == 0u || sh.SLOWF[lane] != 0);
    const bool served = act && !spilled && (!tight_pass || sh.RESK[(knn - 1u) * 64u + lane] != ~0ull);
    if (served) pending = false;
    const bool progress = tight_pass || __ballot(served) != 0ull;
    tight_pass = false;
    wave_sync_lds_nn();  // (the next pass rewrites P, SLOWF and the lists)
    if (!progress) break;  // wave-uniform: a single point's chunks exceed the space
  }
  if (pending) {  // what the plan cannot hold: the lane's own scan into its own slots
    for (uint32_t r = 0; r < knn; r++) sh.RESK[r * 64u + lane] = ~0ull;
    plane_scan_lane(sh, m, lane, px, py, pz, cx, cy, cz, a.radius2, ins);
  }
  if (!in) return;
  // ---- C: the plane ------------------------------------------------------------------------------------------------------
  // ascending distances: the neighbours inside the radius are a prefix of the slots
  uint32_t cnt = 0;
  unsigned long long last = ~0ull;
  if (okrange) {
#pragma unroll 1
    for (uint32_t r = 0; r < knn; r++) {
      const unsigned long long key = sh.RESK[r * 64u + lane];
      if (key == ~0ull || !(__uint_as_float((uint32_t)(key >> 32)) < a.radius2)) break;
      cnt++;
      last = key;
    }
  }
  // the next iteration's bound: all knn slots inside the radius (d_k: of the farthest)
  gprev[i] = (f32x4){px, py, pz, cnt == knn ? sqrtf(__uint_as_float((uint32_t)(last >> 32))) * 1.0001f : __builtin_inff()};
  float4 rc = make_float4(0.f, 0.f, 0.f, 0.f), rn = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cnt >= a.min_pts)
    pl_knn_plane(a, cnt, [&](int r) { return pts4[(uint32_t)sh.RESK[(uint32_t)r * 64u + lane]]; }, px, py, pz, rc, rn);
  G(reinterpret_cast<f32x4*>(pl_c))[i] = (f32x4){rc.x, rc.y, rc.z, rc.w};
  G(reinterpret_cast<f32x4*>(pl_n))[i] = (f32x4){rn.x, rn.y, rn.z, rn.w};
}

}  // namespace mh

// The plane pairs of a LayerTable: pair i owns the workgroups [blk_*[i], blk_*[i + 1]) of the three plane launches (a point pair:
// none), its Gauss-Newton / covariance columns start at blk_acc[i] / blk_cov[i] of the second partials block.
struct PlaneDesc {
  float4 *pl_c, *pl_n;  // this pair's segment
  double plane_eigen_threshold;
  float radius2;
  uint32_t knn, min_pts, pad;
};
struct PlaneTable {
  uint32_t blk_match[MH_MAX_LAYER_PAIRS + 1];
  uint32_t blk_acc[MH_MAX_LAYER_PAIRS + 1];
  uint32_t blk_cov[MH_MAX_LAYER_PAIRS + 1];
  uint32_t pad;
  PlaneDesc d[MH_MAX_LAYER_PAIRS];
};
typedef const PlaneTable __attribute__((address_space(4))) * cplanes_ptr;

// one wave of k_match_layers_pl: workgroup `b` of the table's flattened plane-search range (`cst`: the alignment's state, not
// terminated)
__device__ __forceinline__ void match_layers_pl_wave(mh::FlatWaveP& sh, const clayers_state_ptr cst, const clayers_ptr ct,
                                                     const cplanes_ptr cp, const uint32_t b) {
  const uint32_t li = layer_of(cp->blk_match, ct->n_pairs, b);
  const uint32_t n = ct->d[li].n;
  const uint32_t i0 = (b - cp->blk_match[li]) * kFlatPointsPerBlock + (threadIdx.x & ~63u);
  if (i0 >= n) return;    // whole waves
  const uint32_t iter = cst->iter;
  if (!layer_active(ct, li, iter)) {  // (match_layers_wave: "not paired" for every point of the pair, no bound left behind)
    const uint32_t i = i0 + (uint32_t)__lane_id();
    if (i < n) {
      G(reinterpret_cast<f32x4*>(cp->d[li].pl_c))[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      G(reinterpret_cast<f32x4*>(cp->d[li].pl_n))[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      G(reinterpret_cast<f32x4*>(ct->d[li].pair_q))[i] = (f32x4){0.f, 0.f, 0.f, __builtin_inff()};
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
  PlKnnArg a;
  a.distance_threshold = G(ct->d[li].mk.thr)[iter];
  a.plane_eigen_threshold = cp->d[li].plane_eigen_threshold;
  a.radius2 = cp->d[li].radius2;
  a.knn = cp->d[li].knn;
  a.min_pts = cp->d[li].min_pts;
  mh::match_planes_wave(sh, map, T, a, have_prev, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, n, i0, ct->d[li].pair_q, cp->d[li].pl_c,
                        cp->d[li].pl_n);
}

__global__ __launch_bounds__(kFlatThreads) void k_match_layers_pl(const IcpDeviceState* __restrict__ st,
                                                                  const LayerTable* __restrict__ tab,
                                                                  const PlaneTable* __restrict__ planes) {
  __shared__ mh::FlatWaveP shp[kFlatThreads / 64];
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  match_layers_pl_wave(shp[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(tab), (cplanes_ptr)uniform_const_ptr(planes),
                       blockIdx.x);
}

// the Gauss-Newton rows of the plane pairs' stored pairings (acc_pt2pl_rows with the iteration's robust kernel and the pair's
// weight), a point per lane, into the pair's columns of the second partials block: workgroup `b` of the table's flattened plane
// accumulation range (`cst`: the alignment's state, not terminated; `partials`, `pstride`: the alignment's second block)
__device__ __forceinline__ void accum_layers_pl_block(BlockSum<kGenN>& lds, const clayers_state_ptr cst, const clayers_ptr ct,
                                                      const cplanes_ptr cp, const uint32_t first, double* __restrict__ partials,
                                                      const uint32_t pstride, const uint32_t b) {
  if (!first && cst->inner == 0) return;  // the previous solve already closed this ICP iteration
  const uint32_t li = layer_of(cp->blk_acc, ct->n_pairs, b);
  const uint32_t bx = b - cp->blk_acc[li];
  double T[12];
#pragma unroll
  for (int j = 0; j < 12; j++) T[j] = cst->T[j];
  const double kparam = cst->cur_kparam;
  const uint32_t i = bx * kBlock + threadIdx.x;
  double v[kGenN];
#pragma unroll
  for (int j = 0; j < kGenN; j++) v[j] = 0.0;
  if (i < ct->d[li].n) {
    const float4 c = cp->d[li].pl_c[i];
    if (c.w != 0.f)
      acc_pt2pl_rows(v, T, ct->d[li].lx[i], ct->d[li].ly[i], ct->d[li].lz[i], c, cp->d[li].pl_n[i], ct->d[li].mk.kernel, kparam,
                     ct->d[li].mk.w_pt2pt);
  }
  block_sum_rows<kGenN>(v, lds, partials + cp->blk_acc[li], pstride, bx);
}

__global__ __launch_bounds__(kBlock) void k_accum_layers_pl(const IcpDeviceState* __restrict__ st, const LayerTable* __restrict__ tab,
                                                            const PlaneTable* __restrict__ planes, uint32_t first,
                                                            double* __restrict__ partials, uint32_t pstride) {
  __shared__ BlockSum<kGenN> lds;
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;
  accum_layers_pl_block(lds, cst, (clayers_ptr)uniform_const_ptr(tab), (cplanes_ptr)uniform_const_ptr(planes), first, partials,
                        pstride, blockIdx.x);
}

// ... and their covariance rows (an alignment still running, or whose covariance is done, leaves inside the body)
__device__ __forceinline__ void cov_accum_layers_pl_block(const IcpDeviceState* __restrict__ st, const clayers_ptr ct,
                                                          const cplanes_ptr cp, double* __restrict__ partials, const uint32_t pstride,
                                                          const uint32_t b) {
  const uint32_t li = layer_of(cp->blk_cov, ct->n_pairs, b);
  k_cov_accum_plbuf_body(st, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n, cp->d[li].pl_c, cp->d[li].pl_n,
                         partials + cp->blk_cov[li], pstride, b - cp->blk_cov[li]);
}

__global__ __launch_bounds__(kBlock) void k_cov_accum_layers_pl(const IcpDeviceState* __restrict__ st,
                                                                const LayerTable* __restrict__ tab,
                                                                const PlaneTable* __restrict__ planes, double* __restrict__ partials,
                                                                uint32_t pstride) {
  cov_accum_layers_pl_block(st, (clayers_ptr)uniform_const_ptr(tab), (cplanes_ptr)uniform_const_ptr(planes), partials, pstride,
                            blockIdx.x);
}

// ---- lock-step batches (mh_icp_align_layers_batch_planes) ------------------------------------------------------------------------
// What the plane launches of a group need beside its LayerBatchTable (mh_k_layers.h), job by job in that table's order: the job's
// PlaneTable and second partials block in its own context's memory, that block's columns (= its stride = the job's workgroups in
// the plane accumulation and covariance launches), and the jobs' first workgroups in the two flattened grids (a plane pair's
// covariance range is its accumulation range).  A job without plane points owns no workgroup of these launches.  A table of its
// own, uploaded behind the LayerBatchTable / LayerBatchOptTable only for a group of plane jobs.
struct LayerBatchPlaneJob {
  const PlaneTable* planes;
  double* partb;
  uint32_t tot_acc_pl, pad;
};

struct LayerBatchPlaneTable {
  uint32_t job_blk_match[MH_MAX_LAYER_BATCH_JOBS + 1];  // k_match_layers_pl_b (+ the total)
  uint32_t job_blk_acc[MH_MAX_LAYER_BATCH_JOBS + 1];    // k_accum_layers_pl_b / k_cov_accum_layers_pl_b
  LayerBatchPlaneJob j[MH_MAX_LAYER_BATCH_JOBS];
};

typedef const LayerBatchPlaneTable __attribute__((address_space(4))) * clayer_batch_plane_ptr;

// The three kernels above one level up, as k_match_layers_kb is k_match_layers_k: the job by layer_of over the jobs' prefix
// array, out when it has terminated (nothing of its pl_c / pl_n / pair_q is touched), then the body on the job's own tables,
// state, iteration counter and second partials block with the single call's columns and stride.
__global__ __launch_bounds__(kFlatThreads) void k_match_layers_pl_b(const LayerBatchTable* __restrict__ bt,
                                                                    const LayerBatchPlaneTable* __restrict__ bp) {
  __shared__ mh::FlatWaveP shp[kFlatThreads / 64];
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_plane_ptr cq = (clayer_batch_plane_ptr)uniform_const_ptr(bp);
  const uint32_t ji = layer_of(cq->job_blk_match, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  match_layers_pl_wave(shp[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab),
                       (cplanes_ptr)uniform_const_ptr(cq->j[ji].planes), blockIdx.x - cq->job_blk_match[ji]);
}

__global__ __launch_bounds__(kBlock) void k_accum_layers_pl_b(const LayerBatchTable* __restrict__ bt,
                                                              const LayerBatchPlaneTable* __restrict__ bp, uint32_t first) {
  __shared__ BlockSum<kGenN> lds;
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_plane_ptr cq = (clayer_batch_plane_ptr)uniform_const_ptr(bp);
  const uint32_t ji = layer_of(cq->job_blk_acc, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  accum_layers_pl_block(lds, cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab), (cplanes_ptr)uniform_const_ptr(cq->j[ji].planes),
                        first, cq->j[ji].partb, cq->j[ji].tot_acc_pl, blockIdx.x - cq->job_blk_acc[ji]);
}

__global__ __launch_bounds__(kBlock) void k_cov_accum_layers_pl_b(const LayerBatchTable* __restrict__ bt,
                                                                  const LayerBatchPlaneTable* __restrict__ bp) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_plane_ptr cq = (clayer_batch_plane_ptr)uniform_const_ptr(bp);
  const uint32_t ji = layer_of(cq->job_blk_acc, cb->n_jobs, blockIdx.x);
  cov_accum_layers_pl_block(cb->j[ji].st, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab),
                            (cplanes_ptr)uniform_const_ptr(cq->j[ji].planes), cq->j[ji].partb, cq->j[ji].tot_acc_pl,
                            blockIdx.x - cq->job_blk_acc[ji]);
}

// k_solve_b / k_cov_finalize_b for a group of plane jobs: each job's second block behind its first, in the single call's fixed
// order (k_solve_body / k_cov_finalize_body with partB, nB, nB).  Entry points of their own: k_solve_b and k_cov_finalize_b as
// every other batch launches them read what they always read.
__global__ __launch_bounds__(kSolveThreads) void k_solve_pl_b(const BatchJob* __restrict__ jobs,
                                                              const LayerBatchPlaneTable* __restrict__ bp, uint32_t first) {
  const BatchJob& j = jobs[blockIdx.y];
  const uint32_t cols = first ? j.nbm : j.nba;
  const uint32_t nB = bp->j[blockIdx.y].tot_acc_pl;
  k_solve_body(j.st, j.sk, j.part, cols, cols, nB ? bp->j[blockIdx.y].partb : nullptr, nB, nB, first);
}

__global__ __launch_bounds__(kSolveThreads) void k_cov_finalize_pl_b(const BatchJob* __restrict__ jobs,
                                                                     const LayerBatchPlaneTable* __restrict__ bp) {
  const BatchJob& j = jobs[blockIdx.y];
  const uint32_t nB = bp->j[blockIdx.y].tot_acc_pl;
  k_cov_finalize_body(j.st, 0u, j.part, j.nb, j.nb, nB ? bp->j[blockIdx.y].partb : nullptr, nB, nB);
}
