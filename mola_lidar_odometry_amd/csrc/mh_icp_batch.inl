// mh_icp_batch.inl -- mh_icp_align_batch: many alignments (one per context) from one host thread, jobs of the same kernel chain
// advancing in lock step (one launch per kernel over all jobs), the whole loops of small layers side by side in one launch.
// align_batch_run is the sequence: start every job (AlignJob, deferred uploads), form the lock-step groups, stage and run them,
// then the per-stream remainder and the pairs block.  Included by mh_icp.hip inside its extern "C" block (it launches the *_b
// kernels of that translation unit); mh_icp_layers_batch.inl, included after it, uses its group buffers and stream ordering.

namespace {
// descriptor of one job for the *_b kernels (device pointers only; the pairing-block fields are filled by the caller)
void fill_batch_desc(const AlignJob& j, BatchJob& d) {
  memset(&d, 0, sizeof(d));
  d.st = j.ctx->d_state;
  d.st_b = j.ctx->d_state_b;
  d.serial_base = j.serial_base;
  d.mk = &j.ctx->d_params->mk;
  d.sk = &j.ctx->d_params->sk;
  d.lx = j.scan->x; d.ly = j.scan->y; d.lz = j.scan->z;
  d.n = (uint32_t)j.scan->n;
  d.nb = j.nb;
  d.nba = j.nba;
  d.nbm = j.nbm;
  d.map = j.map->view(*j.sw);
  d.pair_q = j.ctx->pair_q.as<float4>();
  d.pair_gidx = j.ctx->pair_gidx.as<uint32_t>();
  d.part = j.ctx->partials.as<double>();
  if (j.pl) {
    d.partb = j.ctx->partials_b.as<double>();
    d.pl_c = j.ctx->pl_c.as<float4>();
    d.pl_n = j.ctx->pl_n.as<float4>();
  }
  d.sched_dst = j.ctx->sched.as<uint32_t>();
  d.sched_dwords = (uint32_t)(2 * j.nsched_pending);
}

// Work still queued on a job's own stream (asynchronous uploads, filters, de-skew, an earlier alignment) must be
// complete before `lead`'s stream reads that job's scan / state: an event per job, waited for by the leader's stream.
mh_status order_after_stream_of(mh_ctx* lead, mh_ctx* ctx) {
  if (ctx == lead || ctx->stream == lead->stream) return MH_OK;
  if (hipStreamQuery(ctx->stream) == hipSuccess) return MH_OK;  // nothing pending there
  MH_HIP(hipEventRecord(ctx->ev_ready, ctx->stream));
  MH_HIP(hipStreamWaitEvent(lead->stream, ctx->ev_ready, 0));
  return MH_OK;
}
mh_status order_after_job_streams(mh_ctx* lead, const std::vector<AlignJob*>& jobs) {
  for (AlignJob* j : jobs) {
    MH_TRY(map_ready_on(j->map, lead->stream));  // a key-frame update of this job's map still running on its side stream
    MH_TRY(order_after_stream_of(lead, j->ctx));
  }
  (void)hipGetLastError();  // hipStreamQuery's hipErrorNotReady is not an error
  return MH_OK;
}
// (multi-layer jobs: LayersJob::start has made every map ready on its job's own stream, which the leader's then waits for)
mh_status order_after_layers_job_streams(mh_ctx* lead, const std::vector<LayersJob*>& jobs) {
  for (LayersJob* j : jobs) MH_TRY(order_after_stream_of(lead, j->ctx));
  (void)hipGetLastError();
  return MH_OK;
}

// Where the batch's final pairings go: device-side layout of the pairs block (header of per-block counts / offsets for
// the compaction + the block itself unless the caller's block already is device memory).
struct PairsPlan {
  bool want = false;
  int32_t mem = MH_MEM_HOST;
  char* host_block = nullptr;    // caller's block (host kinds)
  char* dev_block = nullptr;     // where the kernels write
  uint32_t* dev_hdr = nullptr;
  size_t total_bytes = 0;
  std::vector<size_t> off;       // byte offset of job i in the block
  std::vector<size_t> hdr_off;   // entry offset of job i's counts in the header
};

mh_status plan_pairs(mh_ctx* lead, const std::vector<AlignJob>& jobs, void* pairs_block, int32_t pairs_mem, PairsPlan& pp) {
  pp.want = pairs_block != nullptr;
  if (!pp.want) return MH_OK;
  pp.mem = pairs_mem;
  pp.off.resize(jobs.size());
  pp.hdr_off.resize(jobs.size());
  size_t bytes = 0, hdr = 0;
  for (size_t i = 0; i < jobs.size(); i++) {
    pp.off[i] = bytes;
    pp.hdr_off[i] = hdr;
    bytes += mh_pairs_block_bytes(jobs[i].scan->n);
    hdr += 2 * (size_t)nblk(jobs[i].scan->n ? jobs[i].scan->n : 1);
  }
  pp.total_bytes = bytes;
  const size_t hdr_bytes = (hdr * 4 + 255) / 256 * 256;
  const size_t need = hdr_bytes + (pairs_mem == MH_MEM_DEVICE ? 0 : bytes);
  if (lead->pairs_stage.bytes < need && lead->pairs_copy_pending) {  // the previous download still reads the old buffer
    MH_HIP(mh::wait_stream(lead->copy_stream));
    lead->pairs_copy_pending = false;
  }
  MH_TRY(lead->pairs_stage.reserve(need));
  pp.dev_hdr = lead->pairs_stage.as<uint32_t>();
  pp.dev_block = pairs_mem == MH_MEM_DEVICE ? (char*)pairs_block : lead->pairs_stage.as<char>() + hdr_bytes;
  pp.host_block = pairs_mem == MH_MEM_DEVICE ? nullptr : (char*)pairs_block;
  if (pairs_mem == MH_MEM_HOST_PINNED && !lead->copy_stream) {
    MH_HIP(hipStreamCreateWithFlags(&lead->copy_stream, hipStreamNonBlocking));
    MH_HIP(hipEventCreateWithFlags(&lead->ev_pairs_ready, hipEventDisableTiming));
    MH_HIP(hipEventCreateWithFlags(&lead->ev_pairs_copied, hipEventDisableTiming));
  }
  return MH_OK;
}

void set_pairs_fields(const PairsPlan& pp, size_t job_index, BatchJob& d) {
  if (!pp.want) return;
  d.cp_counts = pp.dev_hdr + pp.hdr_off[job_index];
  d.cp_out = reinterpret_cast<uint32_t*>(pp.dev_block + pp.off[job_index]);
  d.cp_stride = (uint32_t)(mh_pairs_block_bytes(d.n) / 24);
}

// compaction of every finished job's pairings into the block (descriptors `dj` already on the device) + the download
// `lead` owns the staging buffer, the copy stream and its events (plan_pairs: always the FIRST job's context, which is
// what mh_ctx_synchronize(scans[0]'s context) and the next batch wait on); `s` is the stream the compaction runs on --
// the lock-step group's, which is another context's when job 0 is trivial (same device: events order them).
mh_status finish_pairs(mh_ctx* lead, hipStream_t s, const PairsPlan& pp, const BatchJob* dj, uint32_t A, uint32_t gx_cov) {
  if (!pp.want || A == 0) return MH_OK;
  if (lead->pairs_copy_pending) MH_HIP(hipStreamWaitEvent(s, lead->ev_pairs_copied, 0));  // staging still being read
  hipLaunchKernelGGL(k_count_valid_b, dim3(gx_cov, A), dim3(kBlock), 0, s, dj);
  hipLaunchKernelGGL(k_scan_blocks_b, dim3(1, A), dim3(1024), 0, s, dj);
  hipLaunchKernelGGL(k_compact_b, dim3(gx_cov, A), dim3(kBlock), 0, s, dj);
  MH_HIP(hipGetLastError());
  if (pp.mem == MH_MEM_HOST) {
    MH_HIP(hipMemcpyAsync(pp.host_block, pp.dev_block, pp.total_bytes, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
  } else if (pp.mem == MH_MEM_HOST_PINNED) {
    // on the copy stream: the call returns, the next batch's kernels run while this block travels
    MH_HIP(hipEventRecord(lead->ev_pairs_ready, s));
    MH_HIP(hipStreamWaitEvent(lead->copy_stream, lead->ev_pairs_ready, 0));
    MH_HIP(hipMemcpyAsync(pp.host_block, pp.dev_block, pp.total_bytes, hipMemcpyDeviceToHost, lead->copy_stream));
    MH_HIP(hipEventRecord(lead->ev_pairs_copied, lead->copy_stream));
    lead->pairs_copy_pending = true;
  }
  return MH_OK;
}

// The buffers a lock-step group of A jobs keeps in its lead context: device descriptors (+ `extra` bytes behind them), gathered
// states, and ONE pinned mirror [states | descriptors | extra].  The mirror's pointers hold until the lead's next reserve.
mh_status reserve_group_buffers(mh_ctx* lead, uint32_t A, size_t extra, IcpDeviceState*& h_states, BatchJob*& h_desc) {
  static_assert(sizeof(IcpDeviceState) % 8 == 0 && sizeof(BatchJob) % 8 == 0, "staging layout");
  MH_TRY(lead->batch_desc.reserve(A * sizeof(BatchJob) + extra));
  MH_TRY(lead->batch_states.reserve(A * sizeof(IcpDeviceState)));
  MH_TRY(lead->h_batch.reserve(A * (sizeof(IcpDeviceState) + sizeof(BatchJob)) + extra));
  h_states = lead->h_batch.as<IcpDeviceState>();
  h_desc = reinterpret_cast<BatchJob*>(h_states + A);
  return MH_OK;
}
// what ends a group's chunk: every job's state block gathered and copied into the mirror, on the lead's stream
mh_status gather_states(mh_ctx* lead, const BatchJob* dj, uint32_t A, IcpDeviceState* h_states) {
  hipLaunchKernelGGL(k_gather_states, dim3(A), dim3(256), 0, lead->stream, dj, lead->batch_states.as<IcpDeviceState>());
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(h_states, lead->batch_states.p, A * sizeof(IcpDeviceState), hipMemcpyDeviceToHost, lead->stream));
  return MH_OK;
}

// Lock-step mode: every kernel of an iteration is ONE launch over all jobs of a group (blockIdx.y = job).  The jobs'
// tails fill each other's idle lanes, which concurrent streams do not achieve (HIP maps them onto four hardware queues
// whose kernels mostly run one after the other).  A group = the jobs that run the same kernel chain:
//   quad / plan-scan matcher + k_accum + k_solve (large layers), row matcher with the fused first accumulation (2-12 k
//   points), row matcher + one-workgroup accumulate-and-solve (<= 2 k points: what lidar3d-default.yaml feeds), and the
//   same with Matcher_Point2Plane riding along (lidar3d-ndt.yaml);
// each job keeps its own parameters (iteration budget, schedules, hook check point, prior), state block, termination
// flag and iteration count.  Jobs whose chain has no lock-step form (or that are alone in their group) take the
// per-stream path.
// (the kinds of the matcher chains are their matchers' numbers: K_ROWF = the row matcher with the fused first accumulation)
enum LockstepKind { K_NONE = -1, K_QUAD = (int)Matcher::Quad, K_ROWF = (int)Matcher::Row, K_FLAT = (int)Matcher::Flat, K_STEP = 16, K_STEP_PL };
struct LockstepGroup {  // (movable, not copyable: the admission)
  int kind = K_NONE;
  std::vector<AlignJob*> jobs;
  std::vector<size_t> index;
  mh_ctx* lead = nullptr;
  IcpDeviceState* h_states = nullptr;
  const BatchJob* dj = nullptr;
  uint32_t gx_match = 1, gx_acc = 1, gx_cov = 1, gx_step = 1, enq = 0, prof_n = 0, max_iterations = 0, inner = 1, chunk = 10;
  uint32_t m = 0;  // iterations of the chunk being enqueued
  uint32_t src = 2, par = 0, launches = 0;  // k_step16_b: the state block (2 = canonical) and the partials half the next launch reads; launches so far
  bool cov = false, done = false, auto_chunk = false;
  bool off32 = true;       // K_FLAT: flat_off32 holds for every job and MH_NO_OFF32 is off (k_match_flat_b<true>)
  bool loop_wave = false;  // ... as k_icpw_b (point layers): every job its own workgroups
  uint32_t gx_loopw = 1;   // ... whose launch has this many workgroups per job
  bool loop_now = false;   // k_icp16_b: the group's whole loops in ONE launch (admit_group_loops; cleared when a job's workgroups gave up)
  LoopAdmission loop_adm;  // ... and what it holds of the device's admission count meanwhile
  uint32_t size() const { return (uint32_t)jobs.size(); }
  bool step_chain() const { return kind == K_STEP || kind == K_STEP_PL; }
  bool with_planes() const { return kind == K_STEP_PL; }
};

int lockstep_kind(const Switches& sw, const AlignJob& j, bool batch_prof) {
  if (j.finished || sw.no_lockstep || j.trace || j.prof) return K_NONE;
  // row-kernel layers up to 8 k points: k_step16_b, the chain of a single alignment with the jobs' workgroups side by side -- the
  // same sums in the same order, hence the same bits.  (Round 4 also kept the one-workgroup accumulate-and-solve of round 3 for
  // batches, re-ordered to give those bits: 4 / 8 / 16 sequences 3690 / 4920 / 5770 scans/s against 4092 / 5173 / 5510 this
  // way, NDT pipeline 3966 / 4509 / 3939 against 4780 / 5500 / 5600: removed.)
  if (j.plan.step_chain && !batch_prof) return j.pl ? K_STEP_PL : K_STEP;
  const Matcher m = j.plan.matcher;
  return (j.pl || one_lane(m) || (m == Matcher::Row && !j.plan.fused16)) ? K_NONE : (int)m;
}

// The groups of a batch's started jobs, at most 64 (the jobs of the others, like those left out here, take the per-stream path).
// `one_part`: no MH_LOCKSTEP_GROUPS split (the pairs block is compacted by one launch over one group's jobs).
void form_groups(const Switches& sw, std::vector<AlignJob>& jobs, bool batch_prof, bool one_part, std::vector<LockstepGroup>& kept) {
  std::vector<LockstepGroup> groups;
  for (size_t i = 0; i < jobs.size(); i++) {
    const int k = lockstep_kind(sw, jobs[i], batch_prof);
    if (k == K_NONE) continue;
    const mh_icp_params* q = jobs[i].p;
    LockstepGroup* g = nullptr;
    for (LockstepGroup& c : groups)  // same chain, same device, same loop shape
      if (c.kind == k && c.lead->device == jobs[i].ctx->device && c.inner == q->gn.max_inner_iterations &&
          c.cov == (q->compute_covariance != 0))
        g = &c;
    if (!g) {
      groups.emplace_back();
      g = &groups.back();
      g->kind = k;
      g->lead = jobs[i].ctx;
      g->inner = q->gn.max_inner_iterations;
      g->cov = q->compute_covariance != 0;
      g->chunk = q->poll_every ? q->poll_every : 0;
      g->auto_chunk = q->poll_every == 0;
    }
    // automatic chunks: the group's first chunk is as long as its slowest job expects to run (every job's own estimate:
    // first_chunk) -- jobs that finish earlier leave their blocks at once, so only what lies beyond the LAST job's end is
    // wasted, while every poll in between drains the device for a host round trip (measured with fixed chunks of 10 on 8
    // sequences: 3.1 polls per alignment)
    if (g->auto_chunk && jobs[i].chunk > g->chunk) g->chunk = jobs[i].chunk;
    g->jobs.push_back(&jobs[i]);
    g->index.push_back(i);
    g->max_iterations = q->max_iterations > g->max_iterations ? q->max_iterations : g->max_iterations;
  }
  // a job alone in its group gains nothing from lock step; MH_LOCKSTEP_GROUPS splits the groups further (measured: two
  // groups of the C2 batch overlap one's match launch with the other's short launches for +3 %; default off)
  for (LockstepGroup& g : groups) {
    if (g.jobs.size() < 2) continue;
    uint32_t parts = sw.lockstep_groups;
    if (parts > g.jobs.size() / 2) parts = (uint32_t)(g.jobs.size() / 2);
    if (parts < 1 || one_part) parts = 1;
    for (uint32_t part = 0; part < parts; part++) {
      LockstepGroup h;  // (g's shape: nothing else is set yet)
      h.kind = g.kind; h.inner = g.inner; h.cov = g.cov; h.chunk = g.chunk; h.auto_chunk = g.auto_chunk;
      h.max_iterations = g.max_iterations;
      for (size_t a = 0; a < g.jobs.size(); a++)
        if (a * parts / g.jobs.size() == part) {
          h.jobs.push_back(g.jobs[a]);
          h.index.push_back(g.index[a]);
        }
      h.lead = h.jobs[0]->ctx;
      kept.push_back(std::move(h));
    }
  }
  if (kept.size() > 64) kept.resize(64);
}

// Small layers: the whole loops of the group's jobs in ONE launch (k_icp16_b) when every job's layer has at most kLoopMaxGroups
// groups, a workgroup takes at most kLoopGroupsPerWg of them, and the launch's workgroups are admitted (all resident together,
// beside the one-launch loops of single alignments running on the device).  MH_NO_LOOP16 / MH_NO_LOOP16_BATCH: the chain.
// Sets g.loop_now and completes the jobs' descriptors in the mirror, `h_desc`.
void admit_group_loops(const Switches& sw, LockstepGroup& g, BatchJob* h_desc) {
  mh_ctx* const lead = g.lead;
  const uint32_t A = g.size();
  if (!g.step_chain() || sw.no_loop16 || sw.no_loop16_batch || loop_holdoff(lead->device, 0)) return;
  bool fits = true;
  // k_icpw_b (point layers): every job its own workgroups of 128 points; k_icp16_b (NDT maps, MH_NO_LOOPW): the jobs share
  // kStepMaxWorkgroups workgroups of 32 points, a workgroup taking several groups
  g.loop_wave = !g.with_planes() && loop_wave_enabled(sw, true);
  uint32_t units = 0, gx_w = 1;
  for (uint32_t a = 0; a < A; a++) {
    const uint32_t ng = (h_desc[a].n + kStepPoints - 1) / kStepPoints;
    const uint32_t nw = ng < g.gx_step ? ng : g.gx_step;
    if (g.loop_wave) {
      fits = fits && ng <= kLwMaxGroups && g.jobs[a]->sk.max_iterations > 0;
      const uint32_t w = (ng + kLwGroups - 1) / kLwGroups;
      units += w;
      gx_w = w > gx_w ? w : gx_w;
    } else {
      fits = fits && ng <= kLoopMaxGroups && (nw == 0 || (ng + nw - 1) / nw <= kLoopGroupsPerWg) && g.jobs[a]->sk.max_iterations > 0;
    }
  }
  if (!g.loop_wave) units = kLoopUnitsPerCu * g.gx_step * A;
  if (!fits || !g.loop_adm.admit(sw, lead->device, units)) return;
  g.loop_now = true;
  g.gx_loopw = gx_w;
  for (uint32_t a = 0; a < A; a++) {
    AlignJob& j = *g.jobs[a];
    LoopExchange x;
    if (g.loop_wave) {  // (the lead's stream waits for every job's stream: stage_group)
      g.loop_now = map_ensure_qidx(sw, j.map, lead->stream) == MH_OK && j.map->view(sw).pts_q;
      if (!g.loop_now) break;
      h_desc[a].map = j.map->view(sw);  // (with the sub-voxel index)
    }
    g.loop_now = loop_exchange(j.ctx, lead->stream, j.p->max_iterations * j.p->gn.max_inner_iterations + 1u, x) == MH_OK;
    if (!g.loop_now) break;
    h_desc[a].loop_xa = x.xa;
    h_desc[a].loop_xb = x.xb;
    h_desc[a].loop_serial0 = x.serial0;
    h_desc[a].loop_pad = sw.loop16_test_abandon ? 1u : 0u;
  }
  if (!g.loop_now) g.loop_adm.release();
}

// A group's descriptors and its jobs' deferred [state | params] blocks and schedules, staged in the lead's mirror, uploaded in ONE
// copy and scattered to where each job keeps them; the launch grids; the one-launch loops' admission.  `pp`: the pairs plan when
// this group compacts the batch's pairs block, else null.
mh_status stage_group(const Switches& sw, LockstepGroup& g, const PairsPlan* pp) {
  constexpr size_t kBlockBytes = kParamsOffset + sizeof(IcpDeviceParams);  // one job's [state | params] block
  static_assert(kBlockBytes % 4 == 0, "staging layout");
  const uint32_t A = g.size();
  mh_ctx* lead = g.lead;
  MH_TRY(set_device(lead));
  hipStream_t s = lead->stream;
  MH_TRY(order_after_job_streams(lead, g.jobs));
  size_t stage_bytes = 0;
  for (AlignJob* j : g.jobs) stage_bytes += kBlockBytes + j->nsched_pending * sizeof(double);
  BatchJob* h_desc = nullptr;
  MH_TRY(reserve_group_buffers(lead, A, stage_bytes, g.h_states, h_desc));  // descriptors | staged blocks
  char* h_stage = reinterpret_cast<char*>(h_desc + A);
  size_t off = 0;
  for (uint32_t a = 0; a < A; a++) {
    AlignJob& j = *g.jobs[a];
    BatchJob& d = h_desc[a];
    fill_batch_desc(j, d);
    if (pp) set_pairs_fields(*pp, g.index[a], d);
    d.stage_off = (uint32_t)(off / 4);
    uint32_t bm = (uint32_t)((4ull * d.n + kBlock - 1) / kBlock);  // quad
    if (g.kind == K_ROWF) bm = d.nbm;
    if (g.kind == K_FLAT) {
      bm = nblk_flat(d.n);
      g.off32 = g.off32 && !sw.no_off32 && flat_off32(j.map, d.n);
    }
    if (g.step_chain()) {  // all jobs' workgroups resident at once: kStepMaxWorkgroups shared between them
      const uint32_t cap = kStepMaxWorkgroups / A ? kStepMaxWorkgroups / A : 1u;
      const uint32_t ng = (d.n + kStepPoints - 1) / kStepPoints;
      const uint32_t nw = ng < cap ? ng : cap;
      g.gx_step = nw > g.gx_step ? nw : g.gx_step;
    }
    g.gx_match = bm > g.gx_match ? bm : g.gx_match;
    g.gx_acc = d.nba > g.gx_acc ? d.nba : g.gx_acc;
    g.gx_cov = d.nb > g.gx_cov ? d.nb : g.gx_cov;
    // this job's [state | params] mirror and its schedules into the staging area
    memcpy(h_stage + off, j.ctx->h_state, kBlockBytes);
    memcpy(h_stage + off + kBlockBytes, j.ctx->h_sched.p, j.nsched_pending * sizeof(double));
    off += kBlockBytes + j.nsched_pending * sizeof(double);
    j.defer_upload = false;
  }
  admit_group_loops(sw, g, h_desc);
  // descriptors and staged blocks in ONE copy, then a scatter kernel writes every job's block where it lives
  MH_HIP(hipMemcpyAsync(lead->batch_desc.p, h_desc, A * sizeof(BatchJob) + stage_bytes, hipMemcpyHostToDevice, s));
  g.dj = lead->batch_desc.as<BatchJob>();
  hipLaunchKernelGGL(k_scatter_blocks, dim3(A), dim3(256), 0, s, g.dj,
                     reinterpret_cast<const uint32_t*>(lead->batch_desc.as<char>() + A * sizeof(BatchJob)),
                     (uint32_t)(kBlockBytes / 4));
  return MH_OK;
}

// the whole loops of an admitted group's jobs: one launch
void enqueue_group_loops(LockstepGroup& g) {
  const uint32_t A = g.size();
  g_loop16_runs.fetch_add(A);
  if (g.loop_wave) hipLaunchKernelGGL(k_icpw_b, dim3(g.gx_loopw, A), dim3(kLwThreads), 0, g.lead->stream, g.dj);
  else if (g.with_planes()) hipLaunchKernelGGL(k_icp16_b<true>, dim3(g.gx_step, A), dim3(kSolveThreads), 0, g.lead->stream, g.dj);
  else hipLaunchKernelGGL(k_icp16_b<false>, dim3(g.gx_step, A), dim3(kSolveThreads), 0, g.lead->stream, g.dj);
}

// one ICP iteration of every job of the group; `pr`: events around the match launch (profile == 2)
mh_status enqueue_group_iteration(const Switches& sw, LockstepGroup& g, bool pr) {
  hipStream_t s = g.lead->stream;
  const uint32_t A = g.size();
  if (g.step_chain()) {
    for (uint32_t in = 0; in < g.inner; in++) {
      if (g.with_planes()) hipLaunchKernelGGL(k_step16_b<true>, dim3(g.gx_step, A), dim3(kSolveThreads), 0, s, g.dj, g.src, g.par, 0u, g.launches);
      else hipLaunchKernelGGL(k_step16_b<false>, dim3(g.gx_step, A), dim3(kSolveThreads), 0, s, g.dj, g.src, g.par, 0u, g.launches);
      g.src = g.src == 2u ? 0u : (g.src ^ 1u);
      g.par ^= 1u;
      g.launches++;
    }
    return MH_OK;
  }
  if (pr) MH_HIP(hipEventRecord(g.lead->prof_ev[2 * g.prof_n], s));
  switch (g.kind) {
    case K_ROWF: hipLaunchKernelGGL(k_match16f_b, dim3(g.gx_match, A), dim3(kBlock), 0, s, g.dj); break;
    case K_FLAT:
      hipLaunchKernelGGL(g.off32 ? k_match_flat_b<true> : k_match_flat_b<false>, dim3(g.gx_match, A), dim3(kFlatThreads), 0, s, g.dj);
      count_flat_launches(g.off32 ? 2u : 3u, 1u);  // (no graph on this path: what is issued runs)
      break;
    default: hipLaunchKernelGGL(k_match4_b, dim3(g.gx_match, A), dim3(kBlock), 0, s, g.dj); break;
  }
  if (pr) {
    MH_HIP(hipEventRecord(g.lead->prof_ev[2 * g.prof_n + 1], s));
    g.prof_n++;
  }
  if (g.kind != K_ROWF) hipLaunchKernelGGL(g.kind == K_FLAT ? k_accum_b<true> : k_accum_b<false>, dim3(g.gx_acc, A), dim3(kBlock), 0, s, g.dj, 1u);
  hipLaunchKernelGGL(k_solve_b, dim3(1, A), dim3(kSolveThreads), 0, s, g.dj, 1u);
  for (uint32_t in = 1; in < g.inner; in++) {
    hipLaunchKernelGGL(g.kind == K_FLAT ? k_accum_b<true> : k_accum_b<false>, dim3(g.gx_acc, A), dim3(kBlock), 0, s, g.dj, 0u);
    hipLaunchKernelGGL(k_solve_b, dim3(1, A), dim3(kSolveThreads), 0, s, g.dj, 0u);
  }
  return MH_OK;
}

// what closes a group's chunk: the step chain's pending step, the covariance kernels, the states into the lead's mirror
mh_status enqueue_group_tail(LockstepGroup& g) {
  hipStream_t s = g.lead->stream;
  const uint32_t A = g.size();
  if (g.step_chain() && !g.loop_now) {  // the pending Gauss-Newton step of every job, into the canonical state blocks
    if (g.with_planes()) hipLaunchKernelGGL(k_step16_b<true>, dim3(1, A), dim3(kSolveThreads), 0, s, g.dj, g.src, g.par, 1u, g.launches);
    else hipLaunchKernelGGL(k_step16_b<false>, dim3(1, A), dim3(kSolveThreads), 0, s, g.dj, g.src, g.par, 1u, g.launches);
    g.src = 2;
    g.launches++;
  }
  if (g.cov) {  // no-ops for jobs whose loop has not terminated
    hipLaunchKernelGGL(k_cov_prepare_b, dim3(1, A), dim3(64), 0, s, g.dj);
    hipLaunchKernelGGL(k_cov_accum_b, dim3(g.gx_cov, A), dim3(kBlock), 0, s, g.dj);
    if (g.with_planes()) hipLaunchKernelGGL(k_cov_accum_plbuf_b, dim3(g.gx_cov, A), dim3(kBlock), 0, s, g.dj);
    hipLaunchKernelGGL(k_cov_finalize_b, dim3(1, A), dim3(kSolveThreads), 0, s, g.dj);
  }
  return gather_states(g.lead, g.dj, A, g.h_states);
}

// job `a` of the group has its state in the mirror: into its own context's, and its poll (which ends it once its loop has)
mh_status hand_state_to_job(LockstepGroup& g, size_t a, uint32_t enqueued) {
  AlignJob& j = *g.jobs[a];
  memcpy(j.ctx->h_state, &g.h_states[a], sizeof(IcpDeviceState));
  j.enqueued = enqueued < j.p->max_iterations ? enqueued : j.p->max_iterations;
  return j.poll(true);
}

// Waits for the group's chunk and hands every unfinished job its state; g.done once all have terminated.  After one-launch loops
// of which some were abandoned, the group starts over with the chain's first chunk.
mh_status harvest_group(const Switches& sw, LockstepGroup& g) {
  const hipError_t we = mh::wait_stream(g.lead->stream);
  g.loop_adm.release();
  MH_HIP(we);
  if (g.loop_now) {
    // a job whose workgroups gave up waiting for each other left done == 0 and its canonical state block as uploaded: the
    // group goes on launch by launch (k_step16_b from the start; the jobs that did finish are no-ops there)
    g.loop_now = false;
    bool abandoned = false;
    for (size_t a = 0; a < g.jobs.size(); a++) {
      const IcpDeviceState& h = g.h_states[a];
      if (g.jobs[a]->finished || (h.done && !h.handover_timeouts)) continue;
      abandoned = true;
      g_loop16_fallbacks.fetch_add(1);
      MH_HIP(hipMemsetAsync(&g.jobs[a]->ctx->d_state->handover_timeouts, 0, sizeof(uint32_t) * 10, g.lead->stream));
    }
    if (!abandoned) loop_holdoff(g.lead->device, -1);  // (a clean run ends a streak of abandoned loops)
    if (abandoned) {
      if (!sw.loop16_test_abandon) loop_holdoff(g.lead->device, 1);
      for (size_t a = 0; a < g.jobs.size(); a++) {
        const IcpDeviceState& h = g.h_states[a];
        if (g.jobs[a]->finished || !(h.done && !h.handover_timeouts)) continue;
        MH_TRY(hand_state_to_job(g, a, g.jobs[a]->p->max_iterations));
      }
      g.enq = 0;
      g.src = 2;
      g.par = 0;
      g.launches = 0;
      return MH_OK;  // (not done: the next round enqueues the chain's first chunk)
    }
  }
  g.enq += g.m;
  g.done = true;
  if (g.auto_chunk) g.chunk = 8;  // follow-up chunks
  for (size_t a = 0; a < g.jobs.size(); a++) {
    if (g.jobs[a]->finished) continue;
    MH_TRY(hand_state_to_job(g, a, g.enq));
    g.done = g.done && g.jobs[a]->finished;
  }
  return MH_OK;
}

// The loops of all groups, chunk by chunk until every job has terminated.  `prof_group`: the group whose match launches are timed.
// (Round 4 also built the streaming control of AlignJob::run_streaming for a whole lock-step group -- every job publishing in
// its own progress word, the host following the slowest job still running -- and measured it on 4 / 8 / 16 sequences in one
// process: 4073 / 4904 / 6597 scans/s against 4040 / 5255 / 6560 with the chunks below, NDT pipeline 4475 / 4963 / 5120
// against 4186 / 5120 / 5245.  The spinning leader thread takes a core from the seven threads that queue uploads, filters
// and map updates beside it, and a group's tail is amortised over its jobs anyway.  Removed; single alignments keep it.)
mh_status run_groups(const Switches& sw, std::vector<LockstepGroup>& groups, const LockstepGroup* prof_group) {
  for (;;) {
    bool any = false;
    uint32_t m_max = 0;
    for (LockstepGroup& g : groups) {
      if (g.done) continue;
      any = true;
      g.m = (g.max_iterations - g.enq) < g.chunk ? (g.max_iterations - g.enq) : g.chunk;
      if (g.loop_now) {  // everything in one launch, now
        g.m = g.max_iterations - g.enq;
        enqueue_group_loops(g);
        continue;
      }
      m_max = g.m > m_max ? g.m : m_max;
    }
    if (!any) return MH_OK;
    // one chunk per unfinished group, iteration by iteration across the groups so that their launches interleave
    for (uint32_t it = 0; it < m_max; it++)
      for (LockstepGroup& g : groups)
        if (!g.done && !g.loop_now && it < g.m) MH_TRY(enqueue_group_iteration(sw, g, &g == prof_group));
    for (LockstepGroup& g : groups)
      if (!g.done) MH_TRY(enqueue_group_tail(g));
    for (LockstepGroup& g : groups)
      if (!g.done) MH_TRY(harvest_group(sw, g));
  }
}

// profile == 2: the match step of job 0 = its share of its group's lock-step launches
mh_status profile_share(const LockstepGroup& g, mh_icp_result* r0) {
  float ms = 0.f;
  double sum = 0.0;
  uint32_t live = r0->n_iterations + ((r0->termination_reason == MH_TERM_MAX_ITERATIONS) ? 0u : 1u);
  if (live > g.prof_n) live = g.prof_n;
  for (uint32_t i = 0; i < live; i++) {
    MH_HIP(hipEventElapsedTime(&ms, g.lead->prof_ev[2 * i], g.lead->prof_ev[2 * i + 1]));
    sum += ms;
  }
  r0->n_match_launches = live;
  r0->match_kernel_ms = sum / (double)g.jobs.size();
  r0->total_ms = 0.0;
  return MH_OK;
}

// everything that is not in a lock-step group: one stream per job, chunks enqueued round robin
mh_status run_per_stream(std::vector<AlignJob>& jobs, const std::vector<char>& in_group) {
  for (size_t i = 0; i < jobs.size(); i++)
    if (!in_group[i]) MH_TRY(jobs[i].flush_deferred());
  for (;;) {
    bool any = false;
    for (size_t i = 0; i < jobs.size(); i++)
      if (!in_group[i] && !jobs[i].finished) {
        MH_TRY(jobs[i].enqueue_chunk());
        any = true;
      }
    if (!any) return MH_OK;
    for (size_t i = 0; i < jobs.size(); i++)
      if (!in_group[i]) MH_TRY(jobs[i].poll());
  }
}

// the pairs block of a batch whose jobs did not all run in one group: every job has terminated and its stream is drained, one
// compaction launch over all of them on the first job's stream
mh_status compact_batch_pairs(mh_ctx* lead, const std::vector<AlignJob>& jobs, const PairsPlan& pp) {
  std::vector<size_t> act;
  for (size_t i = 0; i < jobs.size(); i++)
    if (!jobs[i].trivial) act.push_back(i);
  if (act.empty()) return MH_OK;
  MH_TRY(set_device(lead));
  const uint32_t A = (uint32_t)act.size();
  MH_TRY(lead->batch_desc.reserve(A * sizeof(BatchJob)));
  MH_TRY(lead->h_batch.reserve(A * sizeof(BatchJob)));
  BatchJob* h_desc = lead->h_batch.as<BatchJob>();
  uint32_t gx_cov = 1;
  for (uint32_t a = 0; a < A; a++) {
    fill_batch_desc(jobs[act[a]], h_desc[a]);
    set_pairs_fields(pp, act[a], h_desc[a]);
    gx_cov = h_desc[a].nb > gx_cov ? h_desc[a].nb : gx_cov;
  }
  MH_HIP(hipMemcpyAsync(lead->batch_desc.p, h_desc, A * sizeof(BatchJob), hipMemcpyHostToDevice, lead->stream));
  MH_TRY(finish_pairs(lead, lead->stream, pp, lead->batch_desc.as<BatchJob>(), A, gx_cov));
  if (pp.mem != MH_MEM_HOST) MH_HIP(mh::wait_stream(lead->stream));  // h_batch is reused by the next batch
  return MH_OK;
}
}  // namespace

static mh_status align_batch_run(const Switches& sw, size_t n_jobs, const mh_map* const* maps, const mh_scan* const* scans,
                                 const mh_icp_params* params, int32_t params_per_job, const double* T_guesses,
                                 const mh_prior* const* priors, mh_icp_result* results, void* pairs_block, int32_t pairs_mem) {
  MH_REQUIRE(n_jobs == 0 || (maps && scans && params && T_guesses && results), "null argument");
  MH_REQUIRE(!pairs_block || pairs_mem == MH_MEM_HOST || pairs_mem == MH_MEM_DEVICE || pairs_mem == MH_MEM_HOST_PINNED,
             "bad mem space");
  if (n_jobs == 0) return MH_OK;
  auto P = [&](size_t i) { return params_per_job ? &params[i] : params; };
  std::vector<AlignJob> jobs(n_jobs);
  for (size_t i = 0; i < n_jobs; i++) {
    MH_TRY(check_align_args(maps[i], scans[i], P(i), T_guesses + 12 * i, &results[i]));
    for (size_t j = 0; j < i; j++)
      MH_REQUIRE(scans[j]->ctx != scans[i]->ctx, "each job of a batch needs its own context");
    MH_REQUIRE(!pairs_block || scans[i]->ctx->device == scans[0]->ctx->device, "a pairs block needs all jobs on one device");
    // a lock-step group uploads its jobs' blocks in one staged copy.  A batch of ONE job defers as well: a job that uploads at once
    // is planned for streaming control (plan_alignment's auto_control), which only mh_icp_align runs (run_streaming) -- chunked by
    // run_per_stream below, such a job records no event for its poll, which then read the state block before the device wrote it.
    jobs[i].defer_upload = true;
    MH_TRY(jobs[i].start(sw, maps[i], scans[i], P(i), T_guesses + 12 * i, priors ? priors[i] : nullptr, &results[i],
                         nullptr, i));
  }
  mh_ctx* lead0 = scans[0]->ctx;
  PairsPlan pp;
  MH_TRY(set_device(lead0));
  MH_TRY(plan_pairs(lead0, jobs, pairs_block, pairs_mem, pp));
  // profile == 2 times job 0's share of a match kernel of its lock-step group: no events of its own unless it goes the per-stream way
  const bool want_prof = jobs[0].prof && !sw.no_lockstep;
  if (want_prof) jobs[0].prof = false;
  std::vector<LockstepGroup> groups;
  form_groups(sw, jobs, want_prof, pp.want, groups);
  std::vector<char> in_group(n_jobs, 0);
  for (LockstepGroup& g : groups)
    for (size_t i : g.index) in_group[i] = 1;
  if (want_prof && !in_group[0]) jobs[0].prof = true;
  const bool pairs_by_group = pp.want && groups.size() == 1 && groups[0].jobs.size() == (size_t)std::count_if(jobs.begin(), jobs.end(), [](const AlignJob& j) { return !j.finished; });
  if (!groups.empty()) {
    for (LockstepGroup& g : groups) MH_TRY(stage_group(sw, g, pairs_by_group ? &pp : nullptr));
    const bool prof0 = want_prof && groups[0].jobs[0] == &jobs[0];
    MH_TRY(run_groups(sw, groups, prof0 ? &groups[0] : nullptr));
    if (prof0) MH_TRY(profile_share(groups[0], jobs[0].res));
    if (pairs_by_group)
      return finish_pairs(lead0, groups[0].lead->stream, pp, groups[0].dj, groups[0].size(), groups[0].gx_cov);
  }
  MH_TRY(run_per_stream(jobs, in_group));
  if (pp.want) MH_TRY(compact_batch_pairs(lead0, jobs, pp));
  return MH_OK;
}

mh_status mh_icp_align_batch(size_t n_jobs, const mh_map* const* maps, const mh_scan* const* scans,
                             const mh_icp_params* params, int32_t params_per_job, const double* T_guesses,
                             const mh_prior* const* priors, mh_icp_result* results, void* pairs_block, int32_t pairs_mem) {
  const Switches sw = read_switches();
  const mh_status st = align_batch_run(sw, n_jobs, maps, scans, params, params_per_job, T_guesses, priors, results, pairs_block, pairs_mem);
  // MH_DEBUG_VERIFY_BATCH=1 (development): every job once more as a single alignment -- a batch has to give the same bits
  if (st == MH_OK && n_jobs && sw.debug_verify_batch && !pairs_block) {
    for (size_t i = 0; i < n_jobs; i++) {
      mh_icp_result r2;
      const mh_icp_params* q = params_per_job ? &params[i] : params;
      if (align_single(sw, maps[i], scans[i], q, T_guesses + 12 * i, priors ? priors[i] : nullptr, &r2, nullptr, nullptr, MH_MEM_HOST) != MH_OK) continue;
      if (memcmp(r2.T, results[i].T, sizeof(r2.T)) != 0 || r2.n_iterations != results[i].n_iterations) {
        double md = 0;
        for (int k = 0; k < 12; k++) md = fmax(md, fabs(r2.T[k] - results[i].T[k]));
        fprintf(stderr, "[MH_DEBUG_VERIFY_BATCH] job %zu of %zu: n = %zu points, batch %u iterations (reason %u, %u pairs) vs single %u (reason %u, %u pairs), max |dT| %.3e; sizes:",
                i, n_jobs, (size_t)scans[i]->n, results[i].n_iterations, results[i].termination_reason, results[i].n_final_pairs, r2.n_iterations,
                r2.termination_reason, r2.n_final_pairs, md);
        for (size_t k = 0; k < n_jobs; k++) fprintf(stderr, " %zu", (size_t)scans[k]->n);
        fprintf(stderr, "\n");
        // which of the two is unstable?  the batch once more, the single once more
        std::vector<mh_icp_result> again(n_jobs);
        if (align_batch_run(sw, n_jobs, maps, scans, params, params_per_job, T_guesses, priors, again.data(), nullptr, pairs_mem) == MH_OK) {
          mh_icp_result r3;
          (void)align_single(sw, maps[i], scans[i], q, T_guesses + 12 * i, priors ? priors[i] : nullptr, &r3, nullptr, nullptr, MH_MEM_HOST);
          fprintf(stderr, "[MH_DEBUG_VERIFY_BATCH]    second batch == first batch: %d, second batch == single: %d, second single == first single: %d (iterations %u / %u / %u / %u)\n",
                  memcmp(again[i].T, results[i].T, sizeof(r2.T)) == 0, memcmp(again[i].T, r2.T, sizeof(r2.T)) == 0,
                  memcmp(r3.T, r2.T, sizeof(r2.T)) == 0, results[i].n_iterations, again[i].n_iterations, r2.n_iterations, r3.n_iterations);
        }
      }
    }
  }
  return st;
}
