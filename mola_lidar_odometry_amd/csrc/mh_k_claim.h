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

__global__ __launch_bounds__(kBlock) void k_claim_layers(const IcpDeviceState* __restrict__ st, const LayerTable* __restrict__ tab,
                                                         const ClaimTable* __restrict__ claims) {
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const cclaim_ptr cc = (cclaim_ptr)uniform_const_ptr(claims);
  const uint32_t li = layer_of(cc->blk, ct->n_pairs, blockIdx.x);
  if (!layer_active(ct, li, cst->iter)) return;  // (wave-uniform; k_match_layers has left kNoMatch in its whole segment)
  const uint32_t i = (blockIdx.x - cc->blk[li]) * kBlock + threadIdx.x;
  if (i >= layer_entries(ct, li)) return;
  const uint32_t g = G(ct->d[li].pair_gidx)[i];
  if (g == kNoMatch || g >= cc->entries[li]) return;  // (no source index reaches the region's end: mh_map_insert numbers them below n_offered)
  (void)__hip_atomic_fetch_min(G(cc->region[li]) + g, claim_key(cc->epoch0 - cst->iter, li, i), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_resolve_layers(const IcpDeviceState* __restrict__ st, const LayerTable* __restrict__ tab,
                                                           const ClaimTable* __restrict__ claims) {
  const clayers_state_ptr cst = (clayers_state_ptr)uniform_const_ptr(st);
  if (cst->done) return;  // grid-uniform
  const clayers_ptr ct = (clayers_ptr)uniform_const_ptr(tab);
  const cclaim_ptr cc = (cclaim_ptr)uniform_const_ptr(claims);
  const uint32_t li = layer_of(cc->blk, ct->n_pairs, blockIdx.x);
  if (!layer_active(ct, li, cst->iter)) return;  // (wave-uniform; k_match_layers has left kNoMatch in its whole segment)
  const uint32_t i = (blockIdx.x - cc->blk[li]) * kBlock + threadIdx.x;
  if (i >= layer_entries(ct, li)) return;
  uint32_t* const gidx = ct->d[li].pair_gidx;
  const uint32_t g = G(gidx)[i];
  if (g == kNoMatch || g >= cc->entries[li]) return;
  if (G(cc->region[li])[g] == claim_key(cc->epoch0 - cst->iter, li, i)) return;  // the first claim: kept
  uint32_t* const w = reinterpret_cast<uint32_t*>(ct->d[li].pair_q + i) + 3;
  G(w)[0] = G(w)[0] | 0x80000000u;
  G(gidx)[i] = kNoMatch;
}
