// mh_icp_layers.inl -- mh_icp_align_layers: one ICP alignment over several Matcher_Points_DistanceThreshold (map, scan) pairs
// (lidar3d-dual-map.yaml, lidar3d-edges.yaml) with one Gauss-Newton solve.  Included by mh_icp.hip inside its anonymous namespace,
// after AlignJob; the set-up, graph cache and read-back it shares with AlignJob are mh_icp_job.inl's.
//
// One description, one check, several public spellings.  An alignment is described by the ABI's mh_layer_job_planes {n_pairs,
// pairs, opts, gates, knn, planes}: every mh_icp_align_layers* entry point fills one and calls align_layers_as, every
// mh_icp_align_layers_batch* one fills one per job (mh_icp_layers_batch.inl).  LayersView is the only reader of the description
// (the defaults of a NULL array live there), check_layers_job the only holder of the argument rules -- the single call and every
// job of a batch pass it before anything is queued -- and LayersJob sets up what has passed.
//
// Per ICP iteration:  k_match_layers -> k_accum_layers(first) -> k_solve -> [k_accum_layers -> k_solve] x (inner - 1)
// over ALL pairs, whatever their number (mh_k_layers.h); the covariance kernels close the chunk that ends the loop.  With a pair
// whose map points pair once only (mh_icp_align_layers_opts, unique_global): k_claim_layers -> k_resolve_layers behind the match
// (mh_k_claim.h), and the set of such pairs is part of the chunk's graph key.
// Iteration gates (mh_icp_align_layers_gated): data of the uploaded table, tested on the device -- a pair outside its interval
// has its match workgroups store "not paired" instead of searching, and every later kernel of the iteration then finds nothing
// of it.  Nothing about the gates enters the graph key.
// pairingsPerPoint > 1 (mh_icp_align_layers_kbest, mh_k_match_kbest.h): such a pair's segment holds n * k entries and it is searched
// by k_match_layers_k, one more launch per iteration beside k_match_layers; the accumulation and the covariance are then the *_k
// entry points, and the pairs' k are part of the graph key.
// Matcher_Point2Plane on a point layer (mh_icp_align_layers_planes, mh_k_match_planes.h): such a pair owns no workgroup and no
// column of the plain kernels; k_match_layers_pl searches it, k_accum_layers_pl / k_cov_accum_layers_pl put its rows into the second
// partials block that k_solve / k_cov_finalize sum behind the first, and the set of such pairs with their knn is part of the graph key.
// Loop control is AlignJob's chunked one: a chunk of iterations is enqueued (replayed from a captured graph once its shape repeats,
// MH_NO_GRAPH=1: never), the host waits for its event and reads the done flag.

constexpr unsigned long long kLayersGraphTag = 0x4C41594552530000ull;  // "LAYERS": no size of a single alignment's key comes near it

struct LayersLayout {
  size_t seg_q[MH_MAX_LAYER_PAIRS], seg_g[MH_MAX_LAYER_PAIRS];  // byte offsets of each pair's pairing buffers
  size_t pair_bytes = 0;
  uint32_t tot_match = 0, tot_acc = 0, tot_cov = 0;
  uint32_t tot_claim = 0;    // workgroups of k_claim_layers / k_resolve_layers (0: no unique pair, neither is launched)
  uint32_t unique_mask = 0;  // bit i: pair i is unique
  size_t claim_off = 0;      // byte offset of the ClaimTable in layers_tab
  uint32_t tot_match_k = 0;  // workgroups of k_match_layers_k (0: no pair with k > 1; it is not launched, the kernels are the plain ones)
  uint32_t knn_key = 0;      // 4 bits per pair: its k when above 1
  size_t knn_off = 0;        // byte offset of the KnnTable in layers_tab
  uint32_t tot_match_pl = 0; // workgroups of k_match_layers_pl (0: no plane pair; none of the plane kernels is launched)
  uint32_t tot_acc_pl = 0;   // workgroups of k_accum_layers_pl / k_cov_accum_layers_pl = columns of the second partials block
  unsigned long long plane_key = 0;  // 5 bits per pair: its knn when it is a plane pair
  size_t plane_off = 0;      // byte offset of the PlaneTable in layers_tab
  size_t seg_c[MH_MAX_LAYER_PAIRS], seg_n[MH_MAX_LAYER_PAIRS];  // byte offsets of a plane pair's pl_c / pl_n
};

// One multi-layer alignment as its caller describes it: the C ABI's mh_layer_job_planes, read through these accessors and nowhere
// else.  A NULL array, a zero pairings_per_point and a planes array without a plane pair become their defaults HERE.
struct LayersView {
  mh_layer_job_planes d = {};
  uint32_t np() const { return (uint32_t)d.n_pairs; }
  const mh_layer_pair& pair(uint32_t i) const { return d.pairs[i]; }
  bool unique(uint32_t i) const { return d.opts && d.opts[i].unique_global; }
  uint32_t run_from(uint32_t i) const { return d.gates ? d.gates[i].run_from_iteration : 0u; }
  uint32_t run_up_to(uint32_t i) const { return d.gates ? d.gates[i].run_up_to_iteration : 0u; }
  uint32_t kpp(uint32_t i) const { return d.knn && d.knn[i].pairings_per_point ? d.knn[i].pairings_per_point : 1u; }  // >= 1
  mh_layer_pair_plane plane(uint32_t i) const { return d.planes ? d.planes[i] : mh_layer_pair_plane{}; }  // knn 0: a point pair
  uint64_t entries(uint32_t i) const { return (uint64_t)pair(i).scan->n * kpp(i); }  // of pair i's pairing segment
  bool active_in(uint32_t i, uint32_t k) const {  // layer_active (mh_k_layers.h) on the host
    return k >= run_from(i) && (run_up_to(i) == 0 || k <= run_up_to(i));
  }
  // potential_pairings: the layer sizes (times the pairings per point: pcLocal.size() * pairingsPerPoint [U]) of the pairs that
  // are active in ICP iteration k (all of them without gates)
  uint64_t potential_in(uint32_t k) const {
    uint64_t s = 0;
    for (uint32_t i = 0; i < np(); i++) s += active_in(i, k) ? entries(i) : 0;
    return s;
  }
  template <class F>
  bool any(F f) const {
    bool a = false;
    for (uint32_t i = 0; i < np(); i++) a = a || f(i);
    return a;
  }
  bool has_unique() const { return any([&](uint32_t i) { return unique(i); }); }
  bool has_knn() const { return any([&](uint32_t i) { return kpp(i) > 1u; }); }  // a pair with k > 1
  bool has_plane() const { return any([&](uint32_t i) { return plane(i).knn != 0u; }); }
};

// a plane pair's parameters as the KNN + PCA matcher takes them (mh_nn_search_pt2pl_knn)
inline mh_pt2pl_knn_params plane_params(const mh_layer_pair_plane& pl, double distance_threshold) {
  mh_pt2pl_knn_params kp{};
  kp.distance_threshold = distance_threshold;
  kp.plane_eigen_threshold = pl.plane_eigen_threshold;
  kp.search_radius = pl.search_radius;
  kp.knn = pl.knn;
  kp.minimum_plane_points = pl.minimum_plane_points;
  return kp;
}

// One multi-layer alignment from its description to its uploaded [state | parameters | table | schedules]: what a single call and
// a job of a batch share.  The description has passed check_layers_job; everything start() queues goes to the job's own
// context stream.
struct LayersJob {
  mh_ctx* ctx = nullptr;
  LayersView v;
  const mh_icp_params* p = nullptr;
  mh_icp_result* res = nullptr;
  const PlaneTable* ptab = nullptr;  // the pinned mirror of the device's plane table (with a plane pair)
  bool trivial = false;       // nothing to run: the result is complete after start()
  LayersLayout L;
  const LayerTable* tab = nullptr;  // the pinned mirror of the device table (the pairing segments: count_pairs)
  uint32_t chunk = 10;        // iterations of the first chunk

  mh_status start(const Switches& sw, const LayersView& v_, const mh_icp_params* p_, const double T0[12], const mh_prior* prior,
                  mh_icp_result* res_, mh_icp_iter* trace, uint64_t* final_pair_counts);
  uint32_t k_last = 0;        // after finish(): the ICP iteration whose match produced the final pairings
  void finish(uint32_t polls, uint32_t enqueued);
  mh_status count_pairs(const mh_pairs_out* final_pairs, uint64_t* final_pair_counts, int32_t pairs_mem,
                        const mh_pairs_pl_out* final_plane_pairs = nullptr);
  mh_status claims_begin(ClaimTable* ct);
};

// The claim table of this alignment's unique pairs (mh_k_claim.h): a region of the context's table per distinct map among them,
// the flattened range of the two kernels, and the epochs of its iterations.  The table's memory is filled with ones (every
// entry empty) when its block is new and when the epochs have run out; otherwise what earlier alignments left loses by its epoch.
mh_status LayersJob::claims_begin(ClaimTable* ct) {
  memset(ct, 0, sizeof(ClaimTable));
  const uint32_t np = v.np();
  const mh_layer_pair* const pairs = v.d.pairs;
  size_t region_off[MH_MAX_LAYER_PAIRS] = {0}, total = 0;
  for (uint32_t i = 0; i < np; i++) {
    ct->blk[i] = L.tot_claim;
    if (!((L.unique_mask >> i) & 1u)) continue;
    const mh_map* m = pairs[i].map;  // (its size and the pair's entries fit the claim key: check_layers_job)
    uint32_t first = i;
    for (uint32_t j = 0; j < i; j++)
      if (((L.unique_mask >> j) & 1u) && pairs[j].map == m && first == i) first = j;
    if (first == i) {
      region_off[i] = total;
      total += ((size_t)m->n_offered + 31) / 32 * 32;
    } else {
      region_off[i] = region_off[first];
    }
    ct->entries[i] = (uint32_t)m->n_offered;
    L.tot_claim += nblk(v.entries(i));
  }
  ct->blk[np] = L.tot_claim;
  const void* const before = ctx->claims.p;
  MH_TRY(ctx->claims.reserve((total ? total : 32) * sizeof(unsigned long long)));
  const uint32_t mi = p->max_iterations;
  if (ctx->claims.p != before || ctx->claim_epoch < mi) {
    MH_HIP(hipMemsetAsync(ctx->claims.p, 0xFF, ctx->claims.bytes, ctx->stream));
    ctx->claim_epoch = 0xFFFFFFFEu;
  }
  ct->epoch0 = ctx->claim_epoch;
  ctx->claim_epoch -= mi;  // iteration k claims with epoch0 - k, k < max_iterations: the next alignment starts below all of them
  for (uint32_t i = 0; i < np; i++)
    if ((L.unique_mask >> i) & 1u) ct->region[i] = ctx->claims.as<unsigned long long>() + region_off[i];
  return MH_OK;
}

mh_status LayersJob::start(const Switches& sw, const LayersView& v_, const mh_icp_params* p_, const double T0[12],
                           const mh_prior* prior, mh_icp_result* res_, mh_icp_iter* trace, uint64_t* final_pair_counts) {
  v = v_;
  p = p_;
  res = res_;
  const uint32_t np = v.np();
  const mh_layer_pair* const pairs = v.d.pairs;
  ctx = pairs[0].scan->ctx;
  if (final_pair_counts)
    for (uint32_t i = 0; i < np; i++) final_pair_counts[i] = 0;
  // (every pair gated off in iteration 0 is NoPairings there, like no points at all)
  if ((trivial = begin_result(res, p, T0, v.potential_in(0)))) return MH_OK;
  MH_TRY(set_device(ctx));
  MH_TRY(ensure_state(ctx));
  hipStream_t s = ctx->stream;
  // every distinct map: its pending key-frame update, its sub-voxel index (the plan / scan search reads it)
  for (uint32_t i = 0; i < np; i++) {
    bool seen = false;
    for (uint32_t j = 0; j < i; j++) seen = seen || pairs[j].map == pairs[i].map;
    if (seen) continue;
    const mh_map* m = pairs[i].map;
    MH_TRY(map_ready_on(m, s));
    MH_TRY(map_ensure_qidx(sw, m, s));
    if (!m->view(sw).pts_q) return fail(MH_ERR_INTERNAL, "the map's sub-voxel index is missing (mh_icp_align_layers needs it)");
  }
  // layout: a pairing segment per pair (a scan shared by two pairs is paired again for each), flattened grids
  L = LayersLayout();
  const size_t mi = p->max_iterations;
  const size_t tab_bytes = (sizeof(LayerTable) + 255) / 256 * 256;
  const size_t sched_bytes = (1 + (size_t)np) * mi * sizeof(double);  // kernel_param | threshold of pair 0 | ... | pair np-1
  for (uint32_t i = 0; i < np; i++) L.unique_mask |= v.unique(i) ? 1u << i : 0u;
  // (a call without unique pairs uploads the bytes it always did)
  L.claim_off = (tab_bytes + sched_bytes + 255) / 256 * 256;
  for (uint32_t i = 0; i < np; i++) L.knn_key |= v.kpp(i) > 1u ? v.kpp(i) << (4 * i) : 0u;
  L.knn_off = (L.claim_off + sizeof(ClaimTable) + 255) / 256 * 256;
  for (uint32_t i = 0; i < np; i++) L.plane_key |= (unsigned long long)v.plane(i).knn << (5 * i);
  L.plane_off = (L.knn_off + sizeof(KnnTable) + 255) / 256 * 256;
  const size_t up_bytes = L.plane_key ? L.plane_off + sizeof(PlaneTable)
                          : L.knn_key ? L.knn_off + sizeof(KnnTable)
                                      : L.unique_mask ? L.claim_off + sizeof(ClaimTable) : tab_bytes + sched_bytes;
  MH_TRY(ctx->h_layers.reserve(up_bytes));
  MH_TRY(ctx->layers_tab.reserve(up_bytes));
  LayerTable* const tab = ctx->h_layers.as<LayerTable>();
  this->tab = tab;
  memset(tab, 0, sizeof(LayerTable));
  tab->n_pairs = np;
  KnnTable* const kt = reinterpret_cast<KnnTable*>(ctx->h_layers.as<char>() + L.knn_off);  // (written with a pair of k > 1 only)
  if (L.knn_key) memset(kt, 0, sizeof(KnnTable));
  PlaneTable* const pt = reinterpret_cast<PlaneTable*>(ctx->h_layers.as<char>() + L.plane_off);  // (written with a plane pair only)
  if (L.plane_key) memset(pt, 0, sizeof(PlaneTable));
  ptab = L.plane_key ? pt : nullptr;
  for (uint32_t i = 0; i < np; i++) {
    const size_t n = v.entries(i), nn = n ? n : 1;  // (k = 1: the points)
    const bool plane = v.plane(i).knn != 0u;
    const size_t n_flat = (v.kpp(i) > 1u || plane) ? 0 : n, n_flat_k = v.kpp(i) > 1u ? pairs[i].scan->n : 0;
    if (L.plane_key) {
      pt->blk_match[i] = L.tot_match_pl;
      pt->blk_acc[i] = pt->blk_cov[i] = L.tot_acc_pl;
      if (plane) {
        L.tot_match_pl += (uint32_t)((n + kFlatPointsPerBlock - 1) / kFlatPointsPerBlock);
        L.tot_acc_pl += n ? nblk(n) : 0u;
      }
    }
    if (L.knn_key) kt->blk[i] = L.tot_match_k;
    L.tot_match_k += (uint32_t)((n_flat_k + kFlatPointsPerBlock - 1) / kFlatPointsPerBlock);
    L.seg_q[i] = L.pair_bytes;
    L.pair_bytes += (nn * sizeof(float4) + 255) / 256 * 256;
    L.seg_g[i] = L.pair_bytes;
    L.pair_bytes += (nn * sizeof(uint32_t) + 255) / 256 * 256;
    tab->blk_match[i] = L.tot_match;
    tab->blk_acc[i] = L.tot_acc;
    tab->blk_cov[i] = L.tot_cov;
    L.tot_match += (uint32_t)((n_flat + kFlatPointsPerBlock - 1) / kFlatPointsPerBlock);
    L.tot_acc += (n && !plane) ? nblk_acc(n) : 0u;
    L.tot_cov += (n && !plane) ? nblk(n) : 0u;
  }
  for (uint32_t i = 0; i < np; i++) {  // (behind every pair's segments: a table without a plane pair keeps its layout)
    if (!v.plane(i).knn) continue;
    const size_t nn = pairs[i].scan->n ? pairs[i].scan->n : 1;
    L.seg_c[i] = L.pair_bytes;
    L.pair_bytes += (nn * sizeof(float4) + 255) / 256 * 256;
    L.seg_n[i] = L.pair_bytes;
    L.pair_bytes += (nn * sizeof(float4) + 255) / 256 * 256;
  }
  tab->blk_match[np] = L.tot_match;
  tab->blk_acc[np] = L.tot_acc;
  tab->blk_cov[np] = L.tot_cov;
  if (L.knn_key) kt->blk[np] = L.tot_match_k;
  if (L.plane_key) {
    pt->blk_match[np] = L.tot_match_pl;
    pt->blk_acc[np] = pt->blk_cov[np] = L.tot_acc_pl;
    MH_TRY(ctx->partials_b.reserve((size_t)kGenN * (L.tot_acc_pl ? L.tot_acc_pl : 1) * sizeof(double)));
  }
  MH_TRY(ctx->layers_pairs.reserve(L.pair_bytes));
  const uint32_t cols = L.tot_acc > L.tot_cov ? L.tot_acc : L.tot_cov;
  MH_TRY(ctx->partials.reserve((size_t)kGenN * (cols ? cols : 1) * sizeof(double)));
  if (trace) MH_TRY(ctx->trace.reserve(mi * sizeof(mh_icp_iter)));
  double* const h_sched = reinterpret_cast<double*>(ctx->h_layers.as<char>() + tab_bytes);
  double* const d_sched = reinterpret_cast<double*>(ctx->layers_tab.as<char>() + tab_bytes);
  memcpy(h_sched, p->kernel_param, mi * sizeof(double));
  char* const pb = ctx->layers_pairs.as<char>();
  const double deg = 3.14159265358979323846 / 180.0;
  for (uint32_t i = 0; i < np; i++) {
    LayerDesc& d = tab->d[i];
    memcpy(h_sched + (1 + i) * mi, pairs[i].threshold, mi * sizeof(double));
    d.map = pairs[i].map->view(sw);
    d.lx = pairs[i].scan->x;
    d.ly = pairs[i].scan->y;
    d.lz = pairs[i].scan->z;
    d.n = (uint32_t)pairs[i].scan->n;
    d.pair_q = reinterpret_cast<float4*>(pb + L.seg_q[i]);
    d.pair_gidx = reinterpret_cast<uint32_t*>(pb + L.seg_g[i]);
    const double ang = pairs[i].threshold_angular_deg * deg;  // as mh_icp_align computes it
    d.mk.thr = d_sched + (1 + i) * mi;
    d.mk.kparam = d_sched;
    d.mk.ang2 = (float)(ang * ang);
    d.mk.kernel = p->gn.robust_kernel;
    d.mk.w_pt2pt = pairs[i].weight;
    d.col_off = tab->blk_acc[i];
    d.cov_off = tab->blk_cov[i];
    d.run_from = v.run_from(i);
    d.run_up_to = v.run_up_to(i);
    d.kpp = v.kpp(i) > 1u ? v.kpp(i) : 0u;  // (k = 1: the word the table always had there)
    if (v.plane(i).knn) {  // (pair_q: what the next iteration's bound needs; distance threshold: the pair's schedule)
      const mh_pt2pl_knn_params kp = plane_params(v.plane(i), 0.0);
      const PlKnnArg a = pl_knn_arg(&kp);
      PlaneDesc& q = pt->d[i];
      q.pl_c = reinterpret_cast<float4*>(pb + L.seg_c[i]);
      q.pl_n = reinterpret_cast<float4*>(pb + L.seg_n[i]);
      q.plane_eigen_threshold = a.plane_eigen_threshold;
      q.radius2 = a.radius2;
      q.knn = a.knn;
      q.min_pts = a.min_pts;
    }
  }
  if (L.unique_mask) MH_TRY(claims_begin(reinterpret_cast<ClaimTable*>(ctx->h_layers.as<char>() + L.claim_off)));
  MH_HIP(hipMemcpyAsync(ctx->layers_tab.p, ctx->h_layers.p, up_bytes, hipMemcpyHostToDevice, s));
  // the shared state and the solver's parameters: pair 0 stands in where a single value is reported (the trace's threshold)
  const MatchK mk = tab->d[0].mk;
  const SolveK sk = make_solve_params(p, prior, mk, trace ? ctx->trace.as<mh_icp_iter>() : nullptr);
  begin_state(ctx, T0, pairs[0].threshold[0], mk.ang2, p->kernel_param[0]);
  MH_TRY(upload_state_and_params(ctx, mk, sk));
  chunk = first_chunk(p, ctx->layers_predicted);
  return MH_OK;
}

// the result from the state block read back into ctx->h_state once the loop has terminated (PairedRatio over all pairs)
void LayersJob::finish(uint32_t polls, uint32_t enqueued) {
  if (p->poll_every == 0) ctx->layers_predicted = live_iterations(ctx->h_state);
  // the iteration whose match produced the final pairings: the one that terminated the loop, or the last of max_iterations
  k_last = ctx->h_state->n_iterations < p->max_iterations ? ctx->h_state->n_iterations : p->max_iterations - 1;
  read_result(ctx->h_state, p, res, v.potential_in(k_last), L.plane_key ? ctx->h_state->n_pairs_pl : 0u, polls, enqueued);
}

// every pair's final pairings compacted out of its segment (into final_pairs[i] when given) and counted
mh_status LayersJob::count_pairs(const mh_pairs_out* final_pairs, uint64_t* final_pair_counts, int32_t pairs_mem,
                                 const mh_pairs_pl_out* final_plane_pairs) {
  if (!(final_pairs || final_pair_counts || final_plane_pairs) || !res->n_final_pairs) return MH_OK;
  const mh_pairs_out none{};
  const mh_pairs_pl_out none_pl{};
  uint64_t sum = 0;
  const mh_layer_pair* const pairs = v.d.pairs;
  for (uint32_t i = 0; i < v.np(); i++) {
    uint64_t c = 0;
    const uint32_t kpp = v.kpp(i);
    if (v.plane(i).knn && pairs[i].scan->n && v.active_in(i, k_last)) {
      MH_TRY(compact_pl_pairs_of(ctx, ptab->d[i].pl_c, ptab->d[i].pl_n, pairs[i].scan->n,
                                 final_plane_pairs ? &final_plane_pairs[i] : &none_pl, final_plane_pairs ? pairs_mem : MH_MEM_DEVICE, &c));
    } else if (pairs[i].scan->n && v.active_in(i, k_last)) {  // (a pair that is gated off there holds "not paired" throughout)
      MH_TRY(compact_pairs_of(ctx, tab->d[i].pair_gidx, tab->d[i].pair_q, v.entries(i), final_pairs ? &final_pairs[i] : &none,
                              final_pairs ? pairs_mem : MH_MEM_DEVICE, &c));
      // the compaction numbers the ENTRIES: entry e belongs to local point e / k (mh_nn_search_k)
      if (kpp > 1u && c && final_pairs && final_pairs[i].local_idx) {
        if (pairs_mem == MH_MEM_HOST) {
          for (uint64_t e = 0; e < c; e++) final_pairs[i].local_idx[e] /= kpp;
        } else {
          hipLaunchKernelGGL(k_div_idx, dim3(nblk(c)), dim3(kBlock), 0, ctx->stream, final_pairs[i].local_idx, (uint32_t)c, kpp);
          MH_HIP(hipGetLastError());
          MH_HIP(mh::wait_stream(ctx->stream));
        }
      }
    }
    if (final_pair_counts) final_pair_counts[i] = c;
    sum += c;
  }
  if (sum != res->n_final_pairs)
    return fail(MH_ERR_INTERNAL, "pair compaction count mismatch: %llu pairings in the buffers, %u in the last accumulation",
                (unsigned long long)sum, res->n_final_pairs);
  return MH_OK;
}

mh_status align_layers(const Switches& sw, const LayersView& v, const mh_icp_params* p, const double T0[12], const mh_prior* prior,
                       mh_icp_result* res, mh_icp_iter* trace, const mh_pairs_out* final_pairs,
                       const mh_pairs_pl_out* final_plane_pairs, uint64_t* final_pair_counts, int32_t pairs_mem) {
  LayersJob job;
  MH_TRY(job.start(sw, v, p, T0, prior, res, trace, final_pair_counts));
  if (job.trivial) return MH_OK;
  const uint32_t np = v.np();
  mh_ctx* const ctx = job.ctx;
  const LayersLayout& L = job.L;
  hipStream_t s = ctx->stream;
  const LayerTable* const dtab = ctx->layers_tab.as<LayerTable>();
  const ClaimTable* const dclaim = reinterpret_cast<const ClaimTable*>(ctx->layers_tab.as<char>() + L.claim_off);
  const KnnTable* const dknn = reinterpret_cast<const KnnTable*>(ctx->layers_tab.as<char>() + L.knn_off);
  const PlaneTable* const dpl = reinterpret_cast<const PlaneTable*>(ctx->layers_tab.as<char>() + L.plane_off);
  // (the plane pairs' rows: the second partials block of k_solve / k_cov_finalize; without such a pair it is absent as before)
  double* const partb = L.tot_acc_pl ? ctx->partials_b.as<double>() : nullptr;
  const uint32_t nB = L.tot_acc_pl;
  // (a table with a pair of k > 1: the entry points that take the local point of an entry from its k)
  const auto accum = L.knn_key ? k_accum_layers_k : k_accum_layers;
  const auto cov_accum = L.knn_key ? k_cov_accum_layers_k : k_cov_accum_layers;
  double* const part = ctx->partials.as<double>();
  const SolveK* const dsk = &ctx->d_params->sk;
  const uint32_t inner = p->gn.max_inner_iterations;
  uint32_t chunk = job.chunk;
  uint32_t enqueued = 0, polls = 0;
  for (;;) {
    const uint32_t m = (p->max_iterations - enqueued) < chunk ? (p->max_iterations - enqueued) : chunk;
    auto enqueue_kernels = [&]() -> mh_status {
      for (uint32_t j = 0; j < m; j++) {
        if (L.tot_match) hipLaunchKernelGGL(k_match_layers, dim3(L.tot_match), dim3(kFlatThreads), 0, s, ctx->d_state, dtab);
        if (L.tot_match_k)
          hipLaunchKernelGGL(k_match_layers_k, dim3(L.tot_match_k), dim3(kFlatThreads), 0, s, ctx->d_state, dtab, dknn);
        if (L.tot_match_pl)
          hipLaunchKernelGGL(k_match_layers_pl, dim3(L.tot_match_pl), dim3(kFlatThreads), 0, s, ctx->d_state, dtab, dpl);
        if (L.tot_claim) {
          hipLaunchKernelGGL(k_claim_layers, dim3(L.tot_claim), dim3(kBlock), 0, s, ctx->d_state, dtab, dclaim);
          hipLaunchKernelGGL(k_resolve_layers, dim3(L.tot_claim), dim3(kBlock), 0, s, ctx->d_state, dtab, dclaim);
        }
        if (L.tot_acc) hipLaunchKernelGGL(accum, dim3(L.tot_acc), dim3(kBlock), 0, s, ctx->d_state, dtab, 1u, part, L.tot_acc);
        if (nB) hipLaunchKernelGGL(k_accum_layers_pl, dim3(nB), dim3(kBlock), 0, s, ctx->d_state, dtab, dpl, 1u, partb, nB);
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, dsk, (const double*)part, L.tot_acc,
                           L.tot_acc, (const double*)partb, nB, nB, 1u);
        for (uint32_t in = 1; in < inner; in++) {
          if (L.tot_acc) hipLaunchKernelGGL(accum, dim3(L.tot_acc), dim3(kBlock), 0, s, ctx->d_state, dtab, 0u, part, L.tot_acc);
          if (nB) hipLaunchKernelGGL(k_accum_layers_pl, dim3(nB), dim3(kBlock), 0, s, ctx->d_state, dtab, dpl, 0u, partb, nB);
          hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, dsk, (const double*)part, L.tot_acc,
                             L.tot_acc, (const double*)partb, nB, nB, 0u);
        }
      }
      if (p->compute_covariance) {  // no-ops unless the loop has terminated
        hipLaunchKernelGGL(k_cov_prepare, dim3(1), dim3(64), 0, s, ctx->d_state, dsk, 0u);
        if (L.tot_cov) hipLaunchKernelGGL(cov_accum, dim3(L.tot_cov), dim3(kBlock), 0, s, ctx->d_state, dtab, part, L.tot_cov);
        if (nB) hipLaunchKernelGGL(k_cov_accum_layers_pl, dim3(nB), dim3(kBlock), 0, s, ctx->d_state, dtab, dpl, partb, nB);
        hipLaunchKernelGGL(k_cov_finalize, dim3(1), dim3(kSolveThreads), 0, s, ctx->d_state, 0u, (const double*)part, L.tot_cov,
                           L.tot_cov, (const double*)partb, nB, nB);
      }
      (void)hipMemcpyAsync(ctx->h_state, ctx->d_state, sizeof(IcpDeviceState), hipMemcpyDeviceToHost, s);
      return MH_OK;
    };
    // a chunk's launches depend on these sizes and buffers only: through the graph cache, as AlignJob::enqueue_chunk's
    unsigned long long key[32] = {0};
    const unsigned long long kv[] = {kLayersGraphTag | np, m, inner, p->compute_covariance, L.tot_match, L.tot_acc, L.tot_cov,
                                     (unsigned long long)dtab, (unsigned long long)part, (unsigned long long)ctx->d_state,
                                     (unsigned long long)ctx->d_params, (unsigned long long)ctx->h_state};
    static_assert(sizeof(kv) + 10 * sizeof(key[0]) <= sizeof(key), "graph key too small");
    memcpy(key, kv, sizeof(kv));
    if (L.tot_claim) {  // (without a unique pair the key is what it always was)
      unsigned long long* const kc = key + sizeof(kv) / sizeof(kv[0]);
      kc[0] = L.unique_mask;
      kc[1] = L.tot_claim;
      kc[2] = (unsigned long long)dclaim;
    }
    if (L.knn_key) {  // (and without a pair of k > 1)
      unsigned long long* const kk = key + sizeof(kv) / sizeof(kv[0]) + 3;
      kk[0] = L.knn_key;
      kk[1] = L.tot_match_k;
      kk[2] = (unsigned long long)dknn;
    }
    if (L.plane_key) {  // (and without a plane pair)
      unsigned long long* const kq = key + sizeof(kv) / sizeof(kv[0]) + 6;
      kq[0] = L.plane_key;
      kq[1] = ((unsigned long long)L.tot_match_pl << 32) | L.tot_acc_pl;
      kq[2] = (unsigned long long)dpl;
      kq[3] = (unsigned long long)partb;
    }
    MH_TRY(enqueue_cached(ctx, sw.no_graph, key, enqueue_kernels));
    enqueued += m;
    MH_HIP(hipEventRecord(ctx->ev_poll, s));
    polls++;
    MH_HIP(mh::wait_event(ctx->ev_poll));
    if (ctx->h_state->done) break;
    if (enqueued >= p->max_iterations) return fail(MH_ERR_INTERNAL, "device ICP loop did not terminate after max_iterations");
    if (p->poll_every == 0) chunk = kChunkNext;
  }
  job.finish(polls, enqueued);
  if (trace) MH_TRY(download_trace(ctx, ctx->h_state, p, trace));
  return job.count_pairs(final_pairs, final_pair_counts, pairs_mem, v.has_plane() ? final_plane_pairs : nullptr);
}

// Every rule one multi-layer alignment must obey, for the single call and for each job of a batch alike; nothing here touches
// the device, and nothing has been queued when it refuses.  Two passes, because a batch settles the Arguments of ALL its jobs
// before the first Supported rule: MH_ERR_INVALID_ARGUMENT wins over MH_ERR_UNSUPPORTED.  `who` is the public entry point called.
enum class LayerRules { Arguments, Supported };
#define MH_REQUIRE_AS(who, cond, msg)                                                      \
  do {                                                                                     \
    if (!(cond)) return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s", who, msg);                 \
  } while (0)
mh_status check_layers_job(const char* who, LayerRules rules, const LayersView& v, const mh_icp_params* params, const double* T_guess,
                           const mh_icp_result* result) {
  const size_t n_pairs = v.d.n_pairs;
  const mh_layer_pair* const pairs = v.d.pairs;
  if (rules == LayerRules::Arguments) {
    MH_REQUIRE_AS(who, n_pairs >= 1 && n_pairs <= MH_MAX_LAYER_PAIRS, "n_pairs must be 1 .. MH_MAX_LAYER_PAIRS");
    MH_REQUIRE_AS(who, pairs && params && T_guess && result, "null argument");
    for (uint32_t i = 0; i < n_pairs; i++) {
      MH_REQUIRE_AS(who, pairs[i].map && pairs[i].scan && pairs[i].threshold, "null map, scan or threshold in a layer pair");
      MH_REQUIRE_AS(who, pairs[i].map->ctx == pairs[0].scan->ctx && pairs[i].scan->ctx == pairs[0].scan->ctx,
                    "the maps and scans of a multi-layer alignment live on different contexts");
    }
    MH_REQUIRE_AS(who, params->pt2pl_threshold == nullptr, "Matcher_Point2Plane is not supported with layer pairs");
    MH_REQUIRE_AS(who, pose_ok(T_guess), "non-finite initial guess");
    MH_REQUIRE_AS(who, params->max_iterations == 0 || params->kernel_param, "kernel_param array is required");
    MH_REQUIRE_AS(who, params->gn.max_inner_iterations >= 1, "gn.max_inner_iterations must be >= 1");
    MH_REQUIRE_AS(who, params->gn.robust_kernel <= MH_KERNEL_GM_C2, "unknown robust kernel");
    MH_REQUIRE_AS(who, params->max_iterations < (1u << 20), "max_iterations too large");
    MH_REQUIRE_AS(who, params->matched_points <= MH_MATCHED_POINTS_SKIP, "unknown matched_points mode");
    for (uint32_t i = 0; i < n_pairs; i++) {
      MH_REQUIRE_AS(who, v.kpp(i) <= MH_MAX_PAIRINGS_PER_POINT, "pairings_per_point must be 0 .. MH_MAX_PAIRINGS_PER_POINT");
      if (!v.plane(i).knn) continue;
      MH_REQUIRE_AS(who, !v.unique(i), "a plane pair cannot be unique_global");
      MH_REQUIRE_AS(who, v.kpp(i) == 1u, "a plane pair has one pairing per point");
      MH_REQUIRE_AS(who, pairs[i].threshold_angular_deg == 0.0, "a plane pair has no angular threshold");
      for (uint32_t k = 0; k < (params->max_iterations ? params->max_iterations : 1u); k++) {  // (the same code as mh_nn_search_pt2pl_knn's)
        const mh_pt2pl_knn_params kp = plane_params(v.plane(i), params->max_iterations ? pairs[i].threshold[k] : 0.0);
        MH_TRY(check_pl_knn_params(&kp));
      }
    }
    return MH_OK;
  }
  if (params->profile != 0) return fail(MH_ERR_UNSUPPORTED, "%s: profile is not supported", who);
  for (uint32_t i = 0; i < n_pairs; i++) {
    if (params->matched_points == MH_MATCHED_POINTS_SKIP)
      for (uint32_t j = i + 1; j < n_pairs; j++)
        if (pairs[i].scan == pairs[j].scan)
          return fail(MH_ERR_UNSUPPORTED, "%s: MH_MATCHED_POINTS_SKIP with a scan shared by two pairs", who);
    // (n_records: exact once the last (re)build is resolved, an upper bound while it may still run -- never below the truth)
    if (pairs[i].map->n_records >= kFlatMaxRecords) return fail(MH_ERR_UNSUPPORTED, "%s: a map of 2^30 or more records", who);
    if (v.d.knn && v.entries(i) >= (1ull << 32))  // (asked of a job with the array only, as ever)
      return fail(MH_ERR_UNSUPPORTED, "%s: scan size * pairings_per_point does not fit 32 bits", who);
    if (v.unique(i) && v.entries(i) >= kClaimMaxScan)
      return fail(MH_ERR_UNSUPPORTED, "%s: a unique pair with 2^29 or more pairing entries", who);
    if (v.unique(i) && pairs[i].map->n_offered >= kClaimMaxEntries)
      return fail(MH_ERR_UNSUPPORTED, "%s: a unique pair whose map has been offered 2^28 or more points", who);
  }
  return MH_OK;
}

// the single call, under whichever of its five names it was made
mh_status align_layers_as(const char* who, const mh_layer_job_planes& d, const mh_icp_params* params, const double* T_guess,
                          const mh_prior* prior, mh_icp_result* result, mh_icp_iter* trace, const mh_pairs_out* final_pairs,
                          const mh_pairs_pl_out* final_plane_pairs, uint64_t* final_pair_counts, int32_t pairs_mem) {
  const LayersView v{d};
  MH_TRY(check_layers_job(who, LayerRules::Arguments, v, params, T_guess, result));
  MH_REQUIRE_AS(who, !(final_pairs || final_plane_pairs) || pairs_mem == MH_MEM_HOST || pairs_mem == MH_MEM_DEVICE, "bad mem space");
  MH_TRY(check_layers_job(who, LayerRules::Supported, v, params, T_guess, result));
  return align_layers(read_switches(), v, params, T_guess, prior, result, trace, final_pairs, final_plane_pairs, final_pair_counts,
                      pairs_mem);
}
