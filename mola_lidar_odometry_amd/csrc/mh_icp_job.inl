// mh_icp_job.inl -- what every alignment job does on the host around its own kernels, once: AlignJob (mh_icp.hip) and LayersJob
// (mh_icp_layers.inl) set up their result, state block and solver parameters, size their first chunk, replay their chunks from
// the context's graph cache and read their result back through these.  Included by mh_icp.hip inside its anonymous namespace,
// before AlignJob.

// The result before anything has run: the initial guess, cov = diag(1e6), `potential` pairings.  True when nothing is going to
// run (ICP::align with nothing to iterate on: no pairings, quality 0): the result is then complete.
bool begin_result(mh_icp_result* res, const mh_icp_params* p, const double T0[12], uint64_t potential) {
  memset(res, 0, sizeof(*res));
  for (int i = 0; i < 12; i++) res->T[i] = T0[i];
  for (int i = 0; i < 6; i++) res->cov[i * 7] = 1e6;
  res->potential_pairings = potential;
  if (p->max_iterations != 0 && potential != 0) return false;
  res->termination_reason = p->max_iterations == 0 ? MH_TERM_MAX_ITERATIONS : MH_TERM_NO_PAIRINGS;
  return true;
}

// The pinned state block of a new alignment of `ctx` (uploaded by the caller, together with the parameters).  Returns the serial
// number it carries -- k_step16's hand-over: the uploaded block carries this alignment's epoch, every launch one more (a launch
// told what to expect waits for exactly that block: neither the previous alignment's nor the launch before last's will do).
uint32_t begin_state(mh_ctx* ctx, const double T0[12], double thr0, float ang2, double kparam0) {
  ctx->align_serial++;
  init_state(ctx->h_state, T0);
  const uint32_t serial = ((uint32_t)ctx->align_serial & 0x3FFu) << 22;
  ctx->h_state->serial = serial;
  ctx->h_state->cur_thr2 = (float)(thr0 * thr0);
  ctx->h_state->cur_ang2 = ang2;
  ctx->h_state->cur_kparam = kparam0;
  return serial;
}

// The solver's parameter block; `mk`'s schedules are the ones it reports (the trace's threshold), `d_trace` the device trace or null.
SolveK make_solve_params(const mh_icp_params* p, const mh_prior* prior, const MatchK& mk, mh_icp_iter* d_trace) {
  SolveK sk;
  memset(&sk, 0, sizeof(sk));
  sk.max_iterations = p->max_iterations;
  sk.disable_stall = p->disable_stall_test;
  sk.max_inner = p->gn.max_inner_iterations;
  sk.min_step_trans = p->min_abs_step_trans;
  sk.min_step_rot = p->min_abs_step_rot;
  sk.min_delta = p->gn.min_delta;
  sk.max_cost = p->gn.max_cost;
  sk.hook_enabled = p->hook_enabled;
  sk.hook_trans = p->hook_min_trans;
  sk.hook_rot = p->hook_min_rot;
  sk.hook_cos_rot = (p->hook_min_rot > 0.0 && p->hook_min_rot < 3.0) ? cos(p->hook_min_rot) : __builtin_nan("");
  if (p->hook_enabled) {
    Pose C;
    for (int i = 0; i < 12; i++) C.m[i] = p->hook_checkpoint[i];
    const Pose Ci = inverse(C);
    for (int i = 0; i < 12; i++) sk.hook_chk_inv[i] = Ci.m[i];
  }
  fill_prior(sk, prior);
  sk.thr = mk.thr;
  sk.kparam = mk.kparam;
  sk.trace = d_trace;
  sk.gn_trace = nullptr;
  sk.cov_hx = p->cov_findif_xyz;
  sk.cov_ha = p->cov_findif_ang;
  return sk;
}

// Iterations of the first chunk.  Every early-exit launch enqueued beyond the end of the loop costs ~1.5 us of stream time and
// every extra host poll ~25 us, so the first chunk should be as long as the loop will run: the caller's estimate when it has one
// (the odometry driver's calls alternate between short ones that the hook stops and long ones that converge, and it knows which
// kind it is making), else `predicted`, what the context's previous alignment needed (consecutive scans of a sequence converge in
// about as many iterations: one host round trip instead of three).  Later chunks are short (kChunkNext).
uint32_t first_chunk(const mh_icp_params* p, uint32_t predicted) {
  if (p->poll_every) return p->poll_every;
  const uint32_t expect = p->expected_iterations ? p->expected_iterations : predicted;
  return expect ? (expect + kChunkMargin > 64 ? 64u : expect + kChunkMargin) : 10u;
}

// iterations whose launches did work (those enqueued after termination are early-exit no-ops): the next first chunk's size
uint32_t live_iterations(const IcpDeviceState* h) { return h->n_iterations + (h->term_reason == MH_TERM_MAX_ITERATIONS ? 0u : 1u); }

// the result from the state block read back into ctx->h_state once the loop has terminated
void read_result(const IcpDeviceState* h, const mh_icp_params* p, mh_icp_result* res, uint64_t potential, uint32_t n_pairs_pt2pl,
                 uint32_t polls, uint32_t enqueued) {
  res->n_host_polls = polls;
  res->n_enqueued_iterations = enqueued;
  for (int i = 0; i < 12; i++) res->T[i] = h->T[i];
  if (p->compute_covariance)
    for (int i = 0; i < 36; i++) res->cov[i] = h->cov[i];
  res->n_iterations = h->n_iterations;
  res->termination_reason = h->term_reason;
  res->n_final_pairs = h->n_pairs;
  res->n_final_pairs_pt2pl = n_pairs_pt2pl;
  res->potential_pairings = potential;  // every matcher adds its layer size (App.B U6)
  res->quality = (h->n_pairs && potential) ? (double)h->n_pairs / (double)potential : 0.0;  // PairedRatio
  if (h->term_reason == MH_TERM_NO_PAIRINGS)
    for (int i = 0; i < 36; i++) res->cov[i] = (i % 7 == 0) ? 1e6 : 0.0;
}

// the per-iteration records of a terminated loop into the caller's array (max_iterations entries, the unused ones zero)
mh_status download_trace(mh_ctx* ctx, const IcpDeviceState* h, const mh_icp_params* p, mh_icp_iter* trace) {
  const uint32_t cnt = h->n_iterations < p->max_iterations ? h->n_iterations + 1 : p->max_iterations;
  memset(trace, 0, sizeof(mh_icp_iter) * p->max_iterations);
  const uint32_t valid = (h->term_reason == MH_TERM_NO_PAIRINGS || h->term_reason == MH_TERM_SOLVER_ERROR) ? h->n_iterations : cnt;
  if (valid) MH_HIP(hipMemcpy(trace, ctx->trace.p, sizeof(mh_icp_iter) * valid, hipMemcpyDeviceToHost));
  return MH_OK;
}

// The exchange block of a one-launch loop of `ctx` (reserved, and cleared on stream `s`, on first use) and the serial numbers of a
// loop of at most `max_steps` Gauss-Newton steps: the entries of no two loops of a context carry the same number.
struct LoopExchange { void *xa = nullptr, *xb = nullptr; uint32_t serial0 = 0; };
mh_status loop_exchange(mh_ctx* ctx, hipStream_t s, uint32_t max_steps, LoopExchange& x) {
  if (ctx->loop_x.bytes < kLoopExchangeBytes) {
    MH_TRY(ctx->loop_x.reserve(kLoopExchangeBytes));
    (void)hipMemsetAsync(ctx->loop_x.p, 0, kLoopExchangeBytes, s);
  }
  x.xa = ctx->loop_x.p;
  x.xb = ctx->loop_x.as<char>() + 2 * (size_t)kAccN * kLoopRowStride * 16;
  x.serial0 = ctx->loop_serial;
  ctx->loop_serial += max_steps + 2u;
  return MH_OK;
}

// One chunk of a job's launches on its context stream, through the context's ONE graph cache.  The launch sequence only depends
// on sizes and device pointers (the per-alignment values sit in device memory) -- all of them words of `key` -- so it is captured
// once and replayed: one host call per chunk instead of ~4 per iteration.  A shape not seen in an earlier alignment is launched
// directly and remembered; it is captured when a LATER alignment brings it again.  (The real pipeline's ICP layer changes size
// with every scan: capturing and instantiating a graph per alignment cost 0.4 ms each.)  `direct`: no cache (MH_NO_GRAPH=1,
// profiled or streamed launches).
// The plan / scan matcher launches `enqueue` issues are tallied in ctx->flat_issued: issued directly they have gone to the device and
// are counted at once; issued under capture they are recorded beside the key and counted whenever that graph is launched.
template <class Enqueue>
mh_status enqueue_cached(mh_ctx* ctx, bool direct, const unsigned long long (&key)[32], Enqueue&& enqueue) {
  hipStream_t s = ctx->stream;
  ctx->flat_issued[0] = ctx->flat_issued[1] = 0;
  const bool cached = !direct && ctx->graph_exec && memcmp(key, ctx->graph_key, sizeof(key)) == 0;
  const bool candidate = !direct && memcmp(key, ctx->graph_candidate, sizeof(key)) == 0;
  if (!cached && !(candidate && ctx->graph_candidate_align != ctx->align_serial)) {
    if (!direct && !candidate) {
      memcpy(ctx->graph_candidate, key, sizeof(key));
      ctx->graph_candidate_align = ctx->align_serial;
    }
    const mh_status es = enqueue();
    for (uint32_t k = 0; k < 2; k++) count_flat_launches(k, ctx->flat_issued[k]);
    MH_TRY(es);
    MH_HIP(hipGetLastError());
    return MH_OK;
  }
  if (!cached) {
    if (ctx->graph_exec) {
      (void)hipGraphExecDestroy(ctx->graph_exec);
      ctx->graph_exec = nullptr;
    }
    hipGraph_t g = nullptr;
    MH_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const mh_status cs = enqueue();
    const hipError_t ce = hipStreamEndCapture(s, &g);
    if (cs != MH_OK || ce != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      return cs != MH_OK ? cs : fail(MH_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
    }
    const hipError_t ie = hipGraphInstantiate(&ctx->graph_exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) {
      ctx->graph_exec = nullptr;
      return fail(MH_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
    }
    memcpy(ctx->graph_key, key, sizeof(key));
    memcpy(ctx->graph_flat, ctx->flat_issued, sizeof(ctx->graph_flat));
  }
  MH_HIP(hipGraphLaunch(ctx->graph_exec, s));
  for (uint32_t k = 0; k < 2; k++) count_flat_launches(k, ctx->graph_flat[k]);
  return MH_OK;
}
