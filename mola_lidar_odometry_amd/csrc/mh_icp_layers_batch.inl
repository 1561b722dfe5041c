// mh_icp_layers_batch.inl -- mh_icp_align_layers_batch: many multi-layer alignments (one per context) from one host thread.  The three
// entry points (plain, _opts, _planes) are one function, align_layers_batch_as, on jobs described as mh_layer_job_planes: every job
// passes check_layers_job (mh_icp_layers.inl) as a single call does, all jobs' argument rules before the first size limit, and the
// group key is read from the jobs' LayersView.  Jobs of
// the same loop shape (inner steps, covariance) advance in LOCK STEP: k_match_layers_b / k_accum_layers_b / k_cov_accum_layers_b
// walk one flattened range over (job, pair) (mh_k_layers.h), k_solve_b / k_cov_prepare_b / k_cov_finalize_b take a workgroup per
// job.  Every job is set up by LayersJob::start exactly as a single call sets it up, in its own context; its partials keep the
// single call's columns and stride, so its result has that call's bits.
// mh_icp_align_layers_batch_opts: the same with every job's unique pairs, iteration gates and pairings per point (what
// mh_icp_align_layers_kbest takes).  LayersJob::start builds the job's ClaimTable and KnnTable as for a single call; a group with
// such a job uploads a LayerBatchOptTable (mh_k_claim.h) behind its LayerBatchTable and enqueues k_match_layers_kb behind
// k_match_layers_b when a job has a pair with k > 1, and k_claim_layers_b -> k_resolve_layers_b before the first accumulation when
// a job has a unique pair.  A group of the k > 1 kind accumulates through k_accum_layers_kb / k_cov_accum_layers_kb, as the single
// call chooses the *_k entry points.  Gates are data of the jobs' tables.  A group without any of it issues what it always issued.
// mh_icp_align_layers_batch_planes: the same with every job's Matcher_Point2Plane pairs (what mh_icp_align_layers_planes takes).
// Plane jobs form groups of their own.  Such a group uploads a LayerBatchPlaneTable (mh_k_match_planes.h) behind the other tables,
// enqueues k_match_layers_pl_b behind the other searches and k_accum_layers_pl_b behind every point accumulation, and its solve
// and covariance finalisation are k_solve_pl_b / k_cov_finalize_pl_b, which add each job's second partials block behind its first.
// Loop control is align_batch_run's chunked one on the lead job's stream.  The chunks are launched directly, NOT replayed from a
// captured graph: a group's composition changes from batch to batch as sequences end, and a chunk is 1 + 2 * inner launches per
// iteration for ALL jobs where the single calls issue that many each.
// Included by mh_icp.hip inside its extern "C" block, after mh_icp_batch.inl (order_after_layers_job_streams, reserve_group_buffers,
// gather_states).

static mh_status align_layers_lockstep(const std::vector<LayersJob*>& g) {
  const uint32_t A = (uint32_t)g.size();
  mh_ctx* const lead = g[0]->ctx;
  MH_TRY(set_device(lead));
  hipStream_t s = lead->stream;
  MH_TRY(order_after_layers_job_streams(lead, g));
  // [gathered states] | job descriptors of the solve / covariance kernels | the (job, pair) table: pinned mirror and device copy
  // ... and, in a group with a unique pair or a pair of k > 1, the jobs' claim / k-best tables and ranges behind it
  // ... and, in a group of plane jobs, their plane tables, second partials blocks and ranges behind that
  bool with_opts = false, kbest = false, planes = false;
  for (const LayersJob* j : g) {
    with_opts = with_opts || j->L.unique_mask || j->L.knn_key;
    kbest = kbest || j->L.knn_key;
    planes = planes || j->L.plane_key;
  }
  const size_t opt_bytes = with_opts ? sizeof(LayerBatchOptTable) : 0;
  const size_t tab_bytes = sizeof(LayerBatchTable) + opt_bytes + (planes ? sizeof(LayerBatchPlaneTable) : 0);
  const size_t desc_bytes = A * sizeof(BatchJob) + tab_bytes;
  IcpDeviceState* h_states = nullptr;
  BatchJob* h_desc = nullptr;
  MH_TRY(reserve_group_buffers(lead, A, tab_bytes, h_states, h_desc));
  LayerBatchTable* const h_tab = reinterpret_cast<LayerBatchTable*>(h_desc + A);
  LayerBatchOptTable* const h_opt = with_opts ? reinterpret_cast<LayerBatchOptTable*>(h_tab + 1) : nullptr;
  LayerBatchPlaneTable* const h_pl =
      planes ? reinterpret_cast<LayerBatchPlaneTable*>(reinterpret_cast<char*>(h_tab + 1) + opt_bytes) : nullptr;
  static_assert(sizeof(LayerBatchTable) % 8 == 0 && sizeof(LayerBatchOptTable) % 8 == 0, "staging layout");
  memset(h_desc, 0, desc_bytes);
  h_tab->n_jobs = A;
  uint32_t tot_match = 0, tot_acc = 0, tot_cov = 0, tot_claim = 0, tot_match_k = 0, tot_match_pl = 0, tot_acc_pl = 0;
  uint32_t max_iterations = 0, chunk = 0;
  const mh_icp_params* const p0 = g[0]->p;
  const uint32_t inner = p0->gn.max_inner_iterations;
  const bool cov = p0->compute_covariance != 0, auto_chunk = p0->poll_every == 0;
  for (uint32_t a = 0; a < A; a++) {
    const LayersJob& j = *g[a];
    h_tab->job_blk_match[a] = tot_match;
    h_tab->job_blk_acc[a] = tot_acc;
    h_tab->job_blk_cov[a] = tot_cov;
    tot_match += j.L.tot_match;
    tot_acc += j.L.tot_acc;
    tot_cov += j.L.tot_cov;
    if (h_opt) {  // (a job without a unique pair / a pair of k > 1 owns no workgroup of those launches: its address is never read)
      char* const dbase = j.ctx->layers_tab.as<char>();
      h_opt->job_blk_claim[a] = tot_claim;
      h_opt->job_blk_match_k[a] = tot_match_k;
      tot_claim += j.L.tot_claim;
      tot_match_k += j.L.tot_match_k;
      h_opt->j[a].claims = j.L.unique_mask ? reinterpret_cast<const ClaimTable*>(dbase + j.L.claim_off) : nullptr;
      h_opt->j[a].knn = j.L.knn_key ? reinterpret_cast<const KnnTable*>(dbase + j.L.knn_off) : nullptr;
    }
    if (h_pl) {  // (a job without plane points owns no workgroup of the plane launches, and its solve reads no second block)
      h_pl->job_blk_match[a] = tot_match_pl;
      h_pl->job_blk_acc[a] = tot_acc_pl;
      tot_match_pl += j.L.tot_match_pl;
      tot_acc_pl += j.L.tot_acc_pl;
      h_pl->j[a].planes = j.L.plane_key ? reinterpret_cast<const PlaneTable*>(j.ctx->layers_tab.as<char>() + j.L.plane_off) : nullptr;
      h_pl->j[a].partb = j.L.tot_acc_pl ? j.ctx->partials_b.as<double>() : nullptr;
      h_pl->j[a].tot_acc_pl = j.L.tot_acc_pl;
    }
    LayerBatchJob& t = h_tab->j[a];
    t.tab = j.ctx->layers_tab.as<LayerTable>();
    t.st = j.ctx->d_state;
    t.part = j.ctx->partials.as<double>();
    t.tot_acc = j.L.tot_acc;
    t.tot_cov = j.L.tot_cov;
    BatchJob& d = h_desc[a];  // what k_solve_b, k_cov_prepare_b, k_cov_finalize_b and k_gather_states read of it
    d.st = j.ctx->d_state;
    d.sk = &j.ctx->d_params->sk;
    d.part = t.part;
    d.nbm = d.nba = j.L.tot_acc;
    d.nb = j.L.tot_cov;
    max_iterations = j.p->max_iterations > max_iterations ? j.p->max_iterations : max_iterations;
    // automatic chunks: as long as the slowest job expects to run (align_batch_run has the reasoning)
    if (auto_chunk && j.chunk > chunk) chunk = j.chunk;
  }
  if (!auto_chunk) chunk = p0->poll_every;
  h_tab->job_blk_match[A] = tot_match;
  h_tab->job_blk_acc[A] = tot_acc;
  h_tab->job_blk_cov[A] = tot_cov;
  if (h_opt) {
    h_opt->job_blk_claim[A] = tot_claim;
    h_opt->job_blk_match_k[A] = tot_match_k;
  }
  if (h_pl) {
    h_pl->job_blk_match[A] = tot_match_pl;
    h_pl->job_blk_acc[A] = tot_acc_pl;
  }
  MH_HIP(hipMemcpyAsync(lead->batch_desc.p, h_desc, desc_bytes, hipMemcpyHostToDevice, s));
  const BatchJob* const dj = lead->batch_desc.as<BatchJob>();
  const LayerBatchTable* const dt = reinterpret_cast<const LayerBatchTable*>(dj + A);
  const LayerBatchOptTable* const dopt = reinterpret_cast<const LayerBatchOptTable*>(dt + 1);  // (read in a group with such a job only)
  // (read in a group of plane jobs only)
  const LayerBatchPlaneTable* const dpl =
      reinterpret_cast<const LayerBatchPlaneTable*>(reinterpret_cast<const char*>(dt + 1) + opt_bytes);
  // (a group of the k > 1 kind: the entry points that take the local point of an entry from its k, as align_layers chooses them)
  const auto accum = kbest ? k_accum_layers_kb : k_accum_layers_b;
  const auto cov_accum = kbest ? k_cov_accum_layers_kb : k_cov_accum_layers_b;
  // one inner step: the point rows, the plane rows, the solve over both blocks (a group without plane jobs: k_solve_b as ever)
  auto step = [&](uint32_t first) {
    if (tot_acc) hipLaunchKernelGGL(accum, dim3(tot_acc), dim3(kBlock), 0, s, dt, first);
    if (tot_acc_pl) hipLaunchKernelGGL(k_accum_layers_pl_b, dim3(tot_acc_pl), dim3(kBlock), 0, s, dt, dpl, first);
    if (planes) hipLaunchKernelGGL(k_solve_pl_b, dim3(1, A), dim3(kSolveThreads), 0, s, dj, dpl, first);
    else hipLaunchKernelGGL(k_solve_b, dim3(1, A), dim3(kSolveThreads), 0, s, dj, first);
  };
  uint32_t enqueued = 0, polls = 0;
  for (;;) {
    const uint32_t m = (max_iterations - enqueued) < chunk ? (max_iterations - enqueued) : chunk;
    for (uint32_t it = 0; it < m; it++) {
      // (a launch without workgroups is skipped: every pair of the group with k > 1 or a plane pair, nobody unique, no point pair)
      if (tot_match) hipLaunchKernelGGL(k_match_layers_b, dim3(tot_match), dim3(kFlatThreads), 0, s, dt);
      if (tot_match_k) hipLaunchKernelGGL(k_match_layers_kb, dim3(tot_match_k), dim3(kFlatThreads), 0, s, dt, dopt);
      if (tot_match_pl) hipLaunchKernelGGL(k_match_layers_pl_b, dim3(tot_match_pl), dim3(kFlatThreads), 0, s, dt, dpl);
      if (tot_claim) {
        hipLaunchKernelGGL(k_claim_layers_b, dim3(tot_claim), dim3(kBlock), 0, s, dt, dopt);
        hipLaunchKernelGGL(k_resolve_layers_b, dim3(tot_claim), dim3(kBlock), 0, s, dt, dopt);
      }
      step(1u);
      for (uint32_t in = 1; in < inner; in++) step(0u);
    }
    if (cov) {  // no-ops for jobs whose loop has not terminated
      hipLaunchKernelGGL(k_cov_prepare_b, dim3(1, A), dim3(64), 0, s, dj);
      if (tot_cov) hipLaunchKernelGGL(cov_accum, dim3(tot_cov), dim3(kBlock), 0, s, dt);
      if (tot_acc_pl) hipLaunchKernelGGL(k_cov_accum_layers_pl_b, dim3(tot_acc_pl), dim3(kBlock), 0, s, dt, dpl);
      if (planes) hipLaunchKernelGGL(k_cov_finalize_pl_b, dim3(1, A), dim3(kSolveThreads), 0, s, dj, dpl);
      else hipLaunchKernelGGL(k_cov_finalize_b, dim3(1, A), dim3(kSolveThreads), 0, s, dj);
    }
    MH_TRY(gather_states(lead, dj, A, h_states));
    enqueued += m;
    polls++;
    MH_HIP(mh::wait_stream(s));
    bool all_done = true;
    for (uint32_t a = 0; a < A; a++) all_done = all_done && h_states[a].done;
    if (all_done) break;
    if (enqueued >= max_iterations) return fail(MH_ERR_INTERNAL, "device ICP loop did not terminate after max_iterations");
    if (auto_chunk) chunk = kChunkNext;
  }
  for (uint32_t a = 0; a < A; a++) {
    LayersJob& j = *g[a];
    memcpy(j.ctx->h_state, &h_states[a], sizeof(IcpDeviceState));
    j.finish(polls, enqueued < j.p->max_iterations ? enqueued : j.p->max_iterations);
  }
  return MH_OK;
}

// the batch, under whichever of its three names it was made
static mh_status align_layers_batch_as(const char* who, size_t n_jobs, const mh_layer_job_planes* jobs, const mh_icp_params* params,
                                       int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                       mh_icp_result* results, uint64_t* final_pair_counts) {
  MH_REQUIRE_AS(who, n_jobs >= 1 && n_jobs <= MH_MAX_LAYER_BATCH_JOBS, "n_jobs must be 1 .. MH_MAX_LAYER_BATCH_JOBS");
  MH_REQUIRE_AS(who, jobs && params && T_guesses && results, "null argument");
  auto P = [&](size_t i) { return params_per_job ? &params[i] : params; };
  auto ctx_of = [&](size_t i) { return jobs[i].pairs[0].scan->ctx; };
  // everything is checked before anything is queued: after an error no context has seen any work (and no claim epoch is taken)
  LayersView v[MH_MAX_LAYER_BATCH_JOBS];
  for (size_t i = 0; i < n_jobs; i++) {
    v[i].d = jobs[i];
    MH_TRY(check_layers_job(who, LayerRules::Arguments, v[i], P(i), T_guesses + 12 * i, &results[i]));
    for (size_t k = 0; k < i; k++) MH_REQUIRE_AS(who, ctx_of(k) != ctx_of(i), "each job of a batch needs its own context");
    MH_REQUIRE_AS(who, ctx_of(i)->device == ctx_of(0)->device, "the jobs of a batch live on different devices");
  }
  for (size_t i = 0; i < n_jobs; i++)
    MH_TRY(check_layers_job(who, LayerRules::Supported, v[i], P(i), T_guesses + 12 * i, &results[i]));
  const Switches sw = read_switches();
  auto counts_of = [&](size_t i) { return final_pair_counts ? final_pair_counts + i * MH_MAX_LAYER_PAIRS : nullptr; };
  if (final_pair_counts)
    for (size_t i = 0; i < n_jobs * MH_MAX_LAYER_PAIRS; i++) final_pair_counts[i] = 0;
  // lock-step groups: same inner steps, same covariance switch, a pair with k > 1 or none, and a plane pair or none (the launches of
  // a chunk are the same for every job of a group; unique pairs and gates do not change them: a job without a unique pair owns no
  // claim workgroup)
  std::vector<LayersJob> lj(n_jobs);
  std::vector<std::vector<size_t>> groups;
  std::vector<char> in_group(n_jobs, 0);
  if (!sw.no_lockstep) {
    for (size_t i = 0; i < n_jobs; i++) {
      const mh_icp_params* q = P(i);
      if (q->max_iterations == 0 || v[i].potential_in(0) == 0) continue;  // trivial: nothing to run
      std::vector<size_t>* g = nullptr;
      for (auto& c : groups)
        if (P(c[0])->gn.max_inner_iterations == q->gn.max_inner_iterations &&
            (P(c[0])->compute_covariance != 0) == (q->compute_covariance != 0) && v[c[0]].has_knn() == v[i].has_knn() &&
            v[c[0]].has_plane() == v[i].has_plane())
          g = &c;
      if (!g) {
        groups.emplace_back();
        g = &groups.back();
      }
      g->push_back(i);
    }
    for (auto& c : groups)
      if (c.size() >= 2)
        for (size_t i : c) in_group[i] = 1;
  }
  for (auto& c : groups) {
    if (c.size() < 2) continue;  // a job alone in its group gains nothing from lock step
    std::vector<LayersJob*> g;
    for (size_t i : c) {
      MH_TRY(lj[i].start(sw, v[i], P(i), T_guesses + 12 * i, priors ? priors[i] : nullptr, &results[i], nullptr, counts_of(i)));
      g.push_back(&lj[i]);
    }
    MH_TRY(align_layers_lockstep(g));
    for (size_t i : c) MH_TRY(lj[i].count_pairs(nullptr, counts_of(i), MH_MEM_DEVICE));
  }
  for (size_t i = 0; i < n_jobs; i++)
    if (!in_group[i])
      MH_TRY(align_layers(sw, v[i], P(i), T_guesses + 12 * i, priors ? priors[i] : nullptr, &results[i], nullptr, nullptr, nullptr,
                          counts_of(i), MH_MEM_HOST));
  return MH_OK;
}

// Three spellings of one call: each hands its jobs on as mh_layer_job_planes, the arrays it does not take NULL.
mh_status mh_icp_align_layers_batch_planes(size_t n_jobs, const mh_layer_job_planes* jobs, const mh_icp_params* params,
                                           int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                           mh_icp_result* results, uint64_t* final_pair_counts) {
  return align_layers_batch_as(__func__, n_jobs, jobs, params, params_per_job, T_guesses, priors, results, final_pair_counts);
}

mh_status mh_icp_align_layers_batch_opts(size_t n_jobs, const mh_layer_job_opts* jobs, const mh_icp_params* params,
                                         int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                         mh_icp_result* results, uint64_t* final_pair_counts) {
  mh_layer_job_planes jp[MH_MAX_LAYER_BATCH_JOBS];
  for (size_t i = 0; jobs && i < n_jobs && i < MH_MAX_LAYER_BATCH_JOBS; i++)
    jp[i] = mh_layer_job_planes{jobs[i].n_pairs, jobs[i].pairs, jobs[i].opts, jobs[i].gates, jobs[i].knn, nullptr};
  return align_layers_batch_as(__func__, n_jobs, jobs ? jp : nullptr, params, params_per_job, T_guesses, priors, results,
                               final_pair_counts);
}

mh_status mh_icp_align_layers_batch(size_t n_jobs, const mh_layer_job* jobs, const mh_icp_params* params, int32_t params_per_job,
                                    const double* T_guesses, const mh_prior* const* priors, mh_icp_result* results,
                                    uint64_t* final_pair_counts) {
  mh_layer_job_planes jp[MH_MAX_LAYER_BATCH_JOBS];
  for (size_t i = 0; jobs && i < n_jobs && i < MH_MAX_LAYER_BATCH_JOBS; i++)
    jp[i] = mh_layer_job_planes{jobs[i].n_pairs, jobs[i].pairs, nullptr, nullptr, nullptr, nullptr};
  return align_layers_batch_as(__func__, n_jobs, jobs ? jp : nullptr, params, params_per_job, T_guesses, priors, results,
                               final_pair_counts);
}
