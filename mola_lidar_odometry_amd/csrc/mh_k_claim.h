// mh_k_claim.h -- allowMatchAlreadyMatchedGlobalPoints == false on the multi-layer chain (mh_icp_align_layers_opts, U13): a map
// point is paired with at most one local point per ICP iteration, the first one in matching order.  Upstream walks the candidates
// serially and keeps a bit per map point; every candidate makes its attempt unconditionally, so the winner of map point g is the
// candidate with the smallest (pair order, local index) among the unique pairs' candidates that name g -- a minimum, computed here
// by two launches between k_match_layers and the first k_accum_layers of an iteration:
//   k_claim_layers    every accepted pairing of a unique pair: one 64-bit atomicMin of its key into the claim table of its map
//   k_resolve_layers  a pairing whose key is not the table's value has lost: the sign bit of pair_q[i].w is set (k_accum_body<true>
//                     reads the verdict there) and pair_gidx[i] = kNoMatch (the covariance and the compaction read it there);
//                     x, y, z and |w| stay, the next iteration's search bound is made of them
// The kernel boundary is the ordering between the two: no grid synchronisation, no fences.  Integer min only, so the verdict does
// not depend on scheduling.  Both walk a flattened block range over the unique pairs (layer_of, mh_k_layers.h); pairs that are not
// unique own no workgroup of it and neither test nor set claims; a unique pair outside its runFromIteration / runUpToIteration
// interval (layer_active, mh_k_layers.h) leaves both at once: it makes and loses no claims in that iteration.
//
// The claim table: one 64-bit entry per SOURCE INDEX of the map (mh_map_info::n_offered entries) -- the index the pairings report
// and the only name of a map point that match_flat_wave leaves behind (the record's position is not stored); a map that has
// evicted points has more source indices than records, and one of 2^28 or more is refused.  Pairs that share a map share its
// region: claims are per map.  An entry is
//     epoch << 32 | pair order << 29 | local index     (local index * k + rank for a pair with k pairings per point)
// with the epoch DESCENDING: every ICP iteration of every alignment on the context takes a smaller one than all before it, so
// whatever an earlier iteration (or an earlier call, against another map, in a region laid out differently) left in an entry is
// larger than any key of the current iteration and loses the atomicMin like an empty entry (all ones) would.  Chosen over clearing
// the entries through the pairings in a third launch: two launches instead of three per iteration, and nothing map-sized is touched
// per iteration either way -- the table is filled with ones when its buffer is created or grows and when the epochs run out (2^32
// iterations), at the price of 8 bytes per entry instead of 4.
#pragma once

constexpr uint32_t kClaimLocalBits = 29;                  // local index below, pair order (MH_MAX_LAYER_PAIRS = 8: 3 bits) above
constexpr uint64_t kClaimMaxScan = 1ull << kClaimLocalBits;   // (entries: points x pairings per point)
constexpr uint64_t kClaimMaxEntries = 1ull << 28;         // source indices of one map (2 GiB of entries)
static_assert(MH_MAX_LAYER_PAIRS <= (1u << (32 - kClaimLocalBits)), "the pair order does not fit the claim key");

struct ClaimTable {
  uint32_t epoch0, pad;                      // the epoch of ICP iteration k of this alignment is epoch0 - k
  uint32_t blk[MH_MAX_LAYER_PAIRS + 1];      // first workgroup of each pair in the flattened range (a pair that is not unique: none)
  uint32_t entries[MH_MAX_LAYER_PAIRS];      // entries of the pair's region (its map's source indices)
  unsigned long long* region[MH_MAX_LAYER_PAIRS];  // the pair's map's region of the claim table
};

typedef const ClaimTable __attribute__((address_space(4))) * cclaim_ptr;

// the pairing entries of pair li: its points, times its pairings per point (mh_k_match_kbest.h) -- entry e = point * k + rank, so
// with the entry as the key's local field the matching order is (pair, local index, rank) and every candidate of a point makes
// its own attempt
__device__ __forceinline__ uint32_t layer_entries(const clayers_ptr ct, uint32_t li) {
  const uint32_t k = ct->d[li].kpp;
  return ct->d[li].n * (k ? k : 1u);
}

__device__ __forceinline__ unsigned long long claim_key(uint32_t epoch, uint32_t li, uint32_t i) {
  return ((unsigned long long)epoch << 32) | (unsigned long long)((li << kClaimLocalBits) | i);
}

// one workgroup of the claims of an alignment that has not terminated: workgroup `b` of its table's flattened claim range
__device__ __forceinline__ void claim_layers_block(const clayers_state_ptr cst, const clayers_ptr ct, const cclaim_ptr cc,
                                                   const uint32_t b) {
  const uint32_t li = layer_of(cc->blk, ct->n_pairs, b);
  if (!layer_active(ct, li, cst->iter)) return;  // (wave-uniform; k_match_layers has left kNoMatch in its whole segment)
  const uint32_t i = (b - cc->blk[li]) * kBlock + threadIdx.x;
  if (i >= layer_entries(ct, li)) return;
  const uint32_t g = G(ct->d[li].pair_gidx)[i];
  if (g == kNoMatch || g >= cc->entries[li]) return;  // (no source index reaches the region's end: mh_map_insert numbers them below n_offered)
  (void)__hip_atomic_fetch_min(G(cc->region[li]) + g, claim_key(cc->epoch0 - cst->iter, li, i), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// ... and of their resolution, over the same range
__device__ __forceinline__ void resolve_layers_block(const clayers_state_ptr cst, const clayers_ptr ct, const cclaim_ptr cc,
                                                     const uint32_t b) {
  const uint32_t li = layer_of(cc->blk, ct->n_pairs, b);
  if (!layer_active(ct, li, cst->iter)) return;  // (wave-uniform; k_match_layers has left kNoMatch in its whole segment)
  const uint32_t i = (b - cc->blk[li]) * kBlock + threadIdx.x;
  if (i >= layer_entries(ct, li)) return;
  uint32_t* const gidx = ct->d[li].pair_gidx;
  const uint32_t g = G(gidx)[i];
  if (g == kNoMatch || g >= cc->entries[li]) return;
  if (G(cc->region[li])[g] == claim_key(cc->epoch0 - cst->iter, li, i)) return;  // the first claim: kept
  uint32_t* const w = reinterpret_cast<uint32_t*>(ct->d[li].pair_q + i) + 3;
  G(w)[0] = G(w)[0] | 0x80000000u;
  G(gidx)[i] = kNoMatch;
}

__global__ __launch_bounds__(kBlock) void k_claim_layers(const IcpDeviceState* __restrict__ st, const LayerTable* __restrict__ tab,
                                                         const ClaimTable* __restrict__ claims) {
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  claim_layers_block(cst, (clayers_ptr)uniform_const_ptr(tab), (cclaim_ptr)uniform_const_ptr(claims), blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_resolve_layers(const IcpDeviceState* __restrict__ st, const LayerTable* __restrict__ tab,
                                                           const ClaimTable* __restrict__ claims) {
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  resolve_layers_block(cst, (clayers_ptr)uniform_const_ptr(tab), (cclaim_ptr)uniform_const_ptr(claims), blockIdx.x);
}

// ---- lock-step batches (mh_icp_align_layers_batch_opts) ---------------------------------------------------------------------------
// What the claim and the k-best launches of a group need beside its LayerBatchTable (mh_k_layers.h), job by job in that table's
// order: the job's ClaimTable and KnnTable in its own context's memory (null where it has no unique pair / no pair with k > 1:
// such a job owns no workgroup of those launches and the address is never read), and the jobs' first workgroups in the two
// flattened grids.  A table of its own, uploaded only for a group that has a job with an option: LayerBatchTable, its upload and
// the *_layers_b kernels that read it stay what they were.
struct KnnTable;
struct LayerBatchOptJob {
  const ClaimTable* claims;
  const KnnTable* knn;
};

struct LayerBatchOptTable {
  uint32_t job_blk_claim[MH_MAX_LAYER_BATCH_JOBS + 1];    // k_claim_layers_b / k_resolve_layers_b (+ the total)
  uint32_t job_blk_match_k[MH_MAX_LAYER_BATCH_JOBS + 1];  // k_match_layers_kb
  LayerBatchOptJob j[MH_MAX_LAYER_BATCH_JOBS];
};

typedef const LayerBatchOptTable __attribute__((address_space(4))) * clayer_batch_opt_ptr;

// k_claim_layers / k_resolve_layers one level up, as k_match_layers_b is k_match_layers: the job by layer_of over the jobs' prefix
// array, out when it has terminated, then the job's own ClaimTable with the job's own iteration counter.  Keys of different jobs
// never meet: every job's regions lie in its own context's claim table.
__global__ __launch_bounds__(kBlock) void k_claim_layers_b(const LayerBatchTable* __restrict__ bt,
                                                           const LayerBatchOptTable* __restrict__ bo) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_opt_ptr co = (clayer_batch_opt_ptr)uniform_const_ptr(bo);
  const uint32_t ji = layer_of(co->job_blk_claim, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  claim_layers_block(cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab), (cclaim_ptr)uniform_const_ptr(co->j[ji].claims),
                     blockIdx.x - co->job_blk_claim[ji]);
}

__global__ __launch_bounds__(kBlock) void k_resolve_layers_b(const LayerBatchTable* __restrict__ bt,
                                                             const LayerBatchOptTable* __restrict__ bo) {
  const clayer_batch_ptr cb = (clayer_batch_ptr)uniform_const_ptr(bt);
  const clayer_batch_opt_ptr co = (clayer_batch_opt_ptr)uniform_const_ptr(bo);
  const uint32_t ji = layer_of(co->job_blk_claim, cb->n_jobs, blockIdx.x);
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(cb->j[ji].st);
  if (cst->done) return;  // uniform over the job's workgroups
  resolve_layers_block(cst, (clayers_ptr)uniform_const_ptr(cb->j[ji].tab), (cclaim_ptr)uniform_const_ptr(co->j[ji].claims),
                       blockIdx.x - co->job_blk_claim[ji]);
}
