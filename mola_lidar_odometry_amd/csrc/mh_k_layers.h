// mh_k_layers.h -- mh_icp_align_layers: one alignment over several (map, scan) point-layer pairs (lidar3d-dual-map.yaml,
// lidar3d-edges.yaml).  Every pair has a descriptor in a device-resident table; all pairs share ONE IcpDeviceState and their
// partial sums feed ONE k_solve.  The entry points walk a flattened block range: pair i owns the workgroups
// [blk_*[i], blk_*[i + 1]) of each launch.  (Chosen over a blockIdx.y grid -- one row of workgroups per pair, sized by the largest
// pair, the rest exiting at once -- by reasoning, NOT measured: the dual-map scans differ in size several times over, so such a
// grid launches workgroups that do nothing.)  The bodies are the single alignment's, unchanged:
//   k_match_layers    match_flat_wave (the plan / scan search of k_match_flat) with the pair's own threshold and angular term
//   k_accum_layers    k_accum_body<true> with the pair's MatchK (its weight), into its columns of the shared partials
//   k_cov_accum_layers  k_cov_accum_body over the pair's pairings, into its columns of the covariance partials
// k_solve / k_cov_prepare / k_cov_finalize are launched as they are over all columns (fixed order: bitwise reproducible).
// Iteration gates (mh_icp_align_layers_gated): run_from / run_up_to of a pair's descriptor against the state's iteration counter,
// both wave-uniform.  k_match_layers is where a gate acts: a pair outside its interval gets "not paired" stored for every point
// instead of a search, and the accumulation, the covariance and the compaction then find nothing of it in what they read anyway
// (zero columns in every accumulation launch).  An ungated table (both words 0) takes the branches it always took.
//
// mh_icp_align_layers_batch (the *_layers_b entry points): the flattened range one level up.  A device-resident job table holds,
// per job, its own LayerTable (built as for a single call), its state block and its partials; job j owns the workgroups
// [job_blk_*[j], job_blk_*[j + 1]) of each launch and, inside them, pair i of that job the range its own table gives.  A workgroup
// finds its job, leaves at once when that job has terminated, then finds its pair.  Pair i writes the columns of the JOB's partials
// it writes in a single call (stride: the job's total), so k_solve_b / k_cov_finalize_b (a workgroup per job: mh_k_launch.h) add
// the same numbers in the same order and every job ends with the bits of its single call.
// (mh_icp_align_layers_batch_opts: the claim / resolve and k-best entry points of a group, and the table that lets their
// workgroups find (job -> pair), are mh_k_claim.h's and mh_k_match_kbest.h's; mh_icp_align_layers_batch_planes: the plane entry
// points of a group and their table are mh_k_match_planes.h's.)
#pragma once

struct LayerDesc {
  MapView map;
  const float *lx, *ly, *lz;
  float4* pair_q;       // this pair's segment of the pairing buffers (a shared scan is paired again for every pair)
  uint32_t* pair_gidx;
  MatchK mk;            // thr: this pair's threshold schedule; ang2; kernel; w_pt2pt: this pair's weight
  uint32_t n;
  uint32_t col_off;     // first column of its k_accum partials
  uint32_t cov_off;     // first column of its covariance partials
  uint32_t run_from;    // Matcher::runFromIteration / runUpToIteration of this pair (mh_icp_align_layers_gated), 0 = no limit: the
  uint32_t run_up_to;   // pair searches in ICP iteration k iff layer_active(k)
  uint32_t kpp;         // pairingsPerPoint when above 1 (mh_icp_align_layers_kbest, mh_k_match_kbest.h), else 0: the segment holds
};                      // n * kpp entries, entry e of local point e / kpp, and k_match_layers_k searches the pair

struct LayerTable {
  uint32_t n_pairs, pad;
  uint32_t blk_match[MH_MAX_LAYER_PAIRS + 1];  // first workgroup of each pair in the flattened grids (+ the total)
  uint32_t blk_acc[MH_MAX_LAYER_PAIRS + 1];
  uint32_t blk_cov[MH_MAX_LAYER_PAIRS + 1];
  LayerDesc d[MH_MAX_LAYER_PAIRS];
};

typedef const LayerTable __attribute__((address_space(4))) * clayers_ptr;

// the pair that owns workgroup b: the last one whose range starts at or before b (pairs without points own no workgroup)
__device__ __forceinline__ uint32_t layer_of(const uint32_t __attribute__((address_space(4))) * start, uint32_t np, uint32_t b) {
  uint32_t li = 0;
  for (uint32_t k = 1; k < np; k++) li += b >= start[k] ? 1u : 0u;
  return li;
}

// Matcher::match's gate [U]: pair li takes part in ICP iteration `iter`.  Table and iteration are wave-uniform: scalar loads, scalar
// compares.  (from == 0 needs no test of its own: iter >= 0.)
__device__ __forceinline__ bool layer_active(const clayers_ptr ct, uint32_t li, uint32_t iter) {
  const uint32_t from = ct->d[li].run_from, up_to = ct->d[li].run_up_to;
  return iter >= from && (up_to == 0u || iter <= up_to);
}

// one wave of pair-owned matching: workgroup `b` of the table's flattened match range (`cst`: the alignment's state, not terminated)
typedef const IcpDeviceState __attribute__((address_space(4))) * clayers_state_ptr;
__device__ __forceinline__ void match_layers_wave(FlatWave& sh, const clayers_state_ptr cst, const clayers_ptr ct, const uint32_t b) {
  const uint32_t li = layer_of(ct->blk_match, ct->n_pairs, b);
  const uint32_t n = ct->d[li].n;
  const uint32_t i0 = (b - ct->blk_match[li]) * kFlatPointsPerBlock + (threadIdx.x & ~63u);
  if (i0 >= n) return;    // whole waves
  const uint32_t iter = cst->iter;
  if (!layer_active(ct, li, iter)) {
    // A pair outside its iterations neither searches nor contributes: every point "not paired" (the verdict k_accum_body<true>
    // reads in the sign, the index the claims, the covariance and the compaction read), whatever its segment held -- its own last
    // active iteration's pairings or another alignment's.  One streaming store per point; no bound is left behind (|w| = inf).
    const uint32_t i = i0 + (uint32_t)__lane_id();
    if (i < n) {
      G(reinterpret_cast<f32x4*>(ct->d[li].pair_q))[i] = (f32x4){0.f, 0.f, 0.f, -__builtin_inff()};
      G(ct->d[li].pair_gidx)[i] = kNoMatch;
    }
    return;
  }
  // field by field: scalar loads through the constant-space table (a MapView field added in mh_internal.h has to be added here:
  // the static_assert below fails until it is)
  static_assert(sizeof(MapView) == 48, "MapView changed: copy the new field in k_match_layers");
  MapView map;
  map.slots = ct->d[li].map.slots;
  map.pts = ct->d[li].map.pts;
  map.mask = ct->d[li].map.mask;
  map.inv_vs = ct->d[li].map.inv_vs;
  map.vs = ct->d[li].map.vs;
  map.trunc = ct->d[li].map.trunc;
  map.ndt = ct->d[li].map.ndt;
  map.no_prev_bound = ct->d[li].map.no_prev_bound;
  map.pts_q = ct->d[li].map.pts_q;
  // (the first active iteration of a pair finds no pairings of its own in its segment: unbounded, like iteration 0)
  const bool have_prev = iter > ct->d[li].run_from && !map.no_prev_bound;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = cst->T[k];
  const double thr = G(ct->d[li].mk.thr)[iter];
  const float thr2 = (float)(thr * thr);  // what k_solve leaves in cur_thr2 for a single alignment
  match_flat_wave(sh, map, T, thr2, ct->d[li].mk.ang2, have_prev, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, n, i0,
                  ct->d[li].pair_q, ct->d[li].pair_gidx);
}

__global__ __launch_bounds__(kFlatThreads, MH_FLAT_WAVES) void k_match_layers(const IcpDeviceState* __restrict__ st,
                                                                               const LayerTable* __restrict__ tab) {
  __shared__ FlatWave sh[kFlatThreads / 64];
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  match_layers_wave(sh[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(tab), blockIdx.x);
}

__global__ __launch_bounds__(kBlock, MH_ACCUM_WAVES) void k_accum_layers(const IcpDeviceState* __restrict__ st,
                                                                         const LayerTable* __restrict__ tab, uint32_t first,
                                                                         double* __restrict__ partials, uint32_t pstride) {
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t li = layer_of(ct->blk_acc, ct->n_pairs, blockIdx.x);
  k_accum_body<true>(st, first, &tab->d[li].mk, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n, ct->d[li].pair_q,
                     ct->d[li].pair_gidx, partials + ct->d[li].col_off, pstride, blockIdx.x - ct->blk_acc[li]);
}

__global__ __launch_bounds__(kBlock) void k_cov_accum_layers(const IcpDeviceState* __restrict__ st,
                                                             const LayerTable* __restrict__ tab, double* __restrict__ partials,
                                                             uint32_t pstride) {
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t li = layer_of(ct->blk_cov, ct->n_pairs, blockIdx.x);
  k_cov_accum_body(st, 0u, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n, ct->d[li].pair_gidx,
                   partials + ct->d[li].cov_off, pstride, blockIdx.x - ct->blk_cov[li]);
}

// ---- lock-step batches of multi-layer alignments (mh_icp_align_layers_batch) -----------------------------------------------------
// (the job's SolveK and the column counts of its solves travel in the BatchJob array that k_solve_b / k_cov_*_b read)
struct LayerBatchJob {
  const LayerTable* tab;  // the job's own table, in its own context's memory
  IcpDeviceState* st;
  double* part;           // the job's partials: k_accum columns, later the covariance's
  uint32_t tot_acc, tot_cov;  // their strides = the job's workgroups in the accumulation / covariance launches
};

struct LayerBatchTable {
  uint32_t n_jobs, pad;
  uint32_t job_blk_match[MH_MAX_LAYER_BATCH_JOBS + 1];  // first workgroup of each job in the flattened grids (+ the total)
  uint32_t job_blk_acc[MH_MAX_LAYER_BATCH_JOBS + 1];
  uint32_t job_blk_cov[MH_MAX_LAYER_BATCH_JOBS + 1];
  LayerBatchJob j[MH_MAX_LAYER_BATCH_JOBS];
};

typedef const LayerBatchTable __attribute__((address_space(4))) * clayer_batch_ptr;

// (the job of a workgroup: layer_of over the jobs' prefix array -- blockIdx.x and the table are wave-uniform, so the search is
// scalar loads and scalar compares, at most MH_MAX_LAYER_BATCH_JOBS - 1 of them per workgroup)
__global__ __launch_bounds__(kFlatThreads, MH_FLAT_WAVES) void k_match_layers_b(const LayerBatchTable* __restrict__ bt) {
  __shared__ FlatWave sh[kFlatThreads / 64];
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const uint32_t ji = layer_of(cb->job_blk_match, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  match_layers_wave(sh[threadIdx.x >> 6], cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab), blockIdx.x - cb->job_blk_match[ji]);
}

__global__ __launch_bounds__(kBlock, MH_ACCUM_WAVES) void k_accum_layers_b(const LayerBatchTable* __restrict__ bt, uint32_t first) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const uint32_t ji = layer_of(cb->job_blk_acc, cb->n_jobs, blockIdx.x);
  const IcpDeviceState* const st = cb->j[ji].st;
  if (((clayers_state_ptr)uniform_const_ptr(st))->done) return;  // uniform over the job's workgroups
  const LayerTable* const tab = cb->j[ji].tab;
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const uint32_t b = blockIdx.x - cb->job_blk_acc[ji];
  const uint32_t li = layer_of(ct->blk_acc, ct->n_pairs, b);
  k_accum_body<true>(st, first, &tab->d[li].mk, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n, ct->d[li].pair_q,
                     ct->d[li].pair_gidx, cb->j[ji].part + ct->d[li].col_off, cb->j[ji].tot_acc, b - ct->blk_acc[li]);
}

// (a job still running or whose covariance is done leaves inside the body, as in k_cov_accum_layers)
__global__ __launch_bounds__(kBlock) void k_cov_accum_layers_b(const LayerBatchTable* __restrict__ bt) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const uint32_t ji = layer_of(cb->job_blk_cov, cb->n_jobs, blockIdx.x);
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(cb->j[ji].tab);
  const uint32_t b = blockIdx.x - cb->job_blk_cov[ji];
  const uint32_t li = layer_of(ct->blk_cov, ct->n_pairs, b);
  k_cov_accum_body(cb->j[ji].st, 0u, ct->d[li].lx, ct->d[li].ly, ct->d[li].lz, ct->d[li].n, ct->d[li].pair_gidx,
                   cb->j[ji].part + ct->d[li].cov_off, cb->j[ji].tot_cov, b - ct->blk_cov[li]);
}
