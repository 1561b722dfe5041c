// mh_occgrid.hip -- the entry points of include/molahip_occgrid.h: a whole group of key-frames ray-traced
// into the occupancy map at once, the index bounds of its cells, and their projection to a 2-D grid.  The reading is written
// down in the header; the kernels are mh_k_occgrid.h's, the store and its scratch are mh_occmap's (mh_occmap_internal.h).
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/molahip_occgrid.h"
#include "mh_frames_pass.h"
#include "mh_k_occgrid.h"
#include "mh_occmap_internal.h"

using namespace mh;
using namespace mh::occ;

namespace {

// One pass: frames[0 .. nf) (P points, S selected ones, S > 0) folded into the store.  The store is swapped last: a failure
// leaves it as the previous pass left it.
mh_status occ_frames_pass(mh_occmap* o, const mh_map_frame* frames, size_t nf, uint64_t P, uint64_t S, bool staged) {
  const mh_occmap_params& PR = o->params;
  const bool trunc = PR.index_mode == MH_INDEX_TRUNC;
  const uint32_t ray_trace = PR.ray_trace_free_space ? 1u : 0u;
  hipStream_t s = o->ctx->stream;
  const uint32_t B = 256;

  // ---- the pass's one upload: [x | y | z of its points (host arrays only)] prefix array [nf + 1] | frame table [nf]
  const FramesUpload up = frames_upload_layout(nf, P, staged, sizeof(OccFrame));  // (mh_frames_pass.h: the layout, the packing)
  const size_t off_start = up.off_start, off_table = up.off_table, up_bytes = up.bytes;
  MH_TRY(o->f_h.reserve(up_bytes));
  MH_TRY(o->f_up.reserve(up_bytes));
  char* h = o->f_h.as<char>();
  char* d = o->f_up.as<char>();
  uint32_t* h_start = (uint32_t*)(h + off_start);
  OccFrame* h_tab = (OccFrame*)(h + off_table);
  frames_fill_upload<OccFrame>(up, frames, nf, staged, h, d);
  uint64_t sel = 0;  // the prefix array is over the SELECTED points (every decimation-th of each frame)
  for (size_t k = 0; k < nf; k++) {
    const mh_map_frame& fr = frames[k];
    h_start[k] = (uint32_t)sel;
    OccFrame& e = h_tab[k];
    for (int a = 0; a < 3; a++) {
      e.ot[a] = (float)fr.T[4 * a + 3];
      const float sc = e.ot[a] * o->inv_res;
      e.oc[a] = trunc ? (int)sc : (int)floorf(sc);
    }
    sel += (fr.n + PR.decimation - 1) / PR.decimation;
  }
  h_start[nf] = (uint32_t)sel;
  MH_HIP(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s));
  const uint32_t* d_start = (const uint32_t*)(d + off_start);
  const OccFrame* d_tab = (const OccFrame*)(d + off_table);

  // ---- rays of all frames: end cells, work items, their prefix sum
  const uint32_t N = (uint32_t)S;
  MH_TRY(o->ray_e.reserve(S * sizeof(int4)));
  MH_TRY(o->items.reserve(S * sizeof(uint32_t)));
  MH_TRY(o->f_rayf.reserve(S * sizeof(uint32_t)));
  MH_TRY(o->prefix.reserve((S + 1) * sizeof(unsigned long long)));
  MH_TRY(o->counters.reserve(256));
  MH_HIP(hipMemsetAsync(o->counters.p, 0, 256, s));
  hipLaunchKernelGGL(k_occf_rays, dim3(nblk(S, B)), dim3(B), 0, s, d_start, d_tab, (uint32_t)nf, N, PR.decimation, o->inv_res,
                     (uint32_t)trunc, PR.max_range > 0.f ? PR.max_range * PR.max_range : -1.f, ray_trace, o->ray_e.as<int4>(),
                     o->items.as<uint32_t>(), o->f_rayf.as<uint32_t>(), o->counters.as<uint32_t>());
  MH_HIP(hipGetLastError());
  unsigned long long* prefix = o->prefix.as<unsigned long long>();
  {
    auto in = rocprim::make_transform_iterator(o->items.as<uint32_t>(), ToU64());
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, in, prefix, 0ull, (size_t)S, rocprim::plus<unsigned long long>(), s);
    }));
  }
  o->h_rb[1] = o->h_rb[2] = 0;
  MH_HIP(hipMemcpyAsync(&o->h_rb[0], prefix + (S - 1), 8, hipMemcpyDeviceToHost, s));
  MH_HIP(hipMemcpyAsync(&o->h_rb[1], o->items.as<uint32_t>() + (S - 1), 4, hipMemcpyDeviceToHost, s));
  MH_HIP(hipMemcpyAsync(&o->h_rb[2], o->counters.p, 4, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));  // (the mirror is free again behind this)
  const uint64_t total = o->h_rb[0] + (o->h_rb[1] & 0xFFFFFFFFull);
  const uint64_t left_out = o->h_rb[2] & 0xFFFFFFFFull;

  // ---- keys in chunks of at most max_keys_per_pass: sorted with their frames, run lengths over (key, frame)
  uint64_t n_e = 0;  // entries (key, frame << 32 | count), sorted by (key, frame)
  const unsigned long long *ek = nullptr, *ev = nullptr;
  uint32_t n_chunks = 0;
  int acur = 0;
  for (uint64_t g0 = 0; g0 < total; g0 += o->max_keys_per_pass) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(o->max_keys_per_pass, total - g0);
    const bool only = g0 == 0 && cnt == total;
    n_chunks++;
    MH_TRY(o->pk.reserve((size_t)cnt * 8));
    MH_TRY(o->pks.reserve((size_t)cnt * 8));
    MH_TRY(o->f_pf.reserve((size_t)cnt * 4));
    MH_TRY(o->f_pfs.reserve((size_t)cnt * 4));
    MH_TRY(o->head.reserve((size_t)cnt * 4));
    MH_TRY(o->pos.reserve((size_t)cnt * 4));
    MH_TRY(o->rc.reserve((size_t)cnt * 4 + 8));
    unsigned long long *pk = o->pk.as<unsigned long long>(), *pks = o->pks.as<unsigned long long>();
    uint32_t *pf = o->f_pf.as<uint32_t>(), *pfs = o->f_pfs.as<uint32_t>();
    uint32_t *head = o->head.as<uint32_t>(), *pos = o->pos.as<uint32_t>(), *rstart = o->rc.as<uint32_t>();
    hipLaunchKernelGGL(k_occf_keys, dim3(nblk(cnt, B)), dim3(B), 0, s, prefix, o->ray_e.as<int4>(), o->f_rayf.as<uint32_t>(), d_tab,
                       N, ray_trace, (unsigned long long)g0, cnt, pk, pf);
    MH_HIP(hipGetLastError());
    // rocPRIM's radix sort is stable: items of equal key keep the order in which they were generated, frame after frame
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, pk, pks, pf, pfs, (size_t)cnt, 0, 64, s); }));
    hipLaunchKernelGGL(k_occf_pair_heads, dim3(nblk(cnt, B)), dim3(B), 0, s, pks, pfs, cnt, head);
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, head, pos, 0u, (size_t)cnt, rocprim::plus<uint32_t>(), s);
    }));
    hipLaunchKernelGGL(k_occf_pair_runs, dim3(nblk(cnt, B)), dim3(B), 0, s, head, pos, cnt, rstart);
    MH_HIP(hipGetLastError());
    o->h_rb[0] = o->h_rb[1] = 0;
    MH_HIP(hipMemcpyAsync(&o->h_rb[0], pos + (cnt - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(&o->h_rb[1], head + (cnt - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    const uint64_t n_runs = (o->h_rb[0] & 0xFFFFFFFFull) + (o->h_rb[1] & 0xFFFFFFFFull);
    if (only) {  // the only chunk: its runs are the entries
      MH_TRY(o->f_ek.reserve(n_runs * 8));
      MH_TRY(o->f_ev.reserve(n_runs * 8));
      hipLaunchKernelGGL(k_occf_entries, dim3(nblk(n_runs, B)), dim3(B), 0, s, pks, pfs, rstart, (uint32_t)n_runs,
                         o->f_ek.as<unsigned long long>(), o->f_ev.as<unsigned long long>());
      MH_HIP(hipGetLastError());
      ek = o->f_ek.as<unsigned long long>();
      ev = o->f_ev.as<unsigned long long>();
      n_e = n_runs;
      break;
    }
    // several chunks: the entries are appended (growing buffers keep no content: copy over), summed after the last one
    MH_REQUIRE(n_e + n_runs < 0x7FFFFFF0ull, "too many (cell, frame) entries in one pass");
    // ONE capacity in entries for the three arrays: the smallest of what each of them holds (their blocks need not have grown in
    // step: DevBuf::reserve rounds by size class and may fall back to the bare need under memory pressure)
    const size_t have = std::min(o->f_ak[acur].bytes / 8, std::min(o->f_af[acur].bytes, o->f_ac[acur].bytes) / 4);
    if (n_e + n_runs > have) {
      const size_t cap = 2 * (size_t)(n_e + n_runs);
      MH_TRY(o->f_ak[acur ^ 1].reserve(cap * 8));
      MH_TRY(o->f_af[acur ^ 1].reserve(cap * 4));
      MH_TRY(o->f_ac[acur ^ 1].reserve(cap * 4));
      if (n_e) {
        MH_HIP(hipMemcpyAsync(o->f_ak[acur ^ 1].p, o->f_ak[acur].p, n_e * 8, hipMemcpyDeviceToDevice, s));
        MH_HIP(hipMemcpyAsync(o->f_af[acur ^ 1].p, o->f_af[acur].p, n_e * 4, hipMemcpyDeviceToDevice, s));
        MH_HIP(hipMemcpyAsync(o->f_ac[acur ^ 1].p, o->f_ac[acur].p, n_e * 4, hipMemcpyDeviceToDevice, s));
      }
      acur ^= 1;
    }
    hipLaunchKernelGGL(k_occf_entries_split, dim3(nblk(n_runs, B)), dim3(B), 0, s, pks, pfs, rstart, (uint32_t)n_runs,
                       o->f_ak[acur].as<unsigned long long>() + n_e, o->f_af[acur].as<uint32_t>() + n_e,
                       o->f_ac[acur].as<uint32_t>() + n_e);
    MH_HIP(hipGetLastError());
    n_e += n_runs;
  }
  if (n_chunks > 1) {
    // The appended entries of ONE key are in frame order already: the chunks follow the work items, and those are generated frame
    // after frame.  A stable sort by key therefore orders them by (key, frame); it runs twice with the same keys, once carrying the
    // frames and once the counts (a stable sort moves equal keys the same way both times).  Equal (key, frame) are then summed.
    const uint32_t NE = (uint32_t)n_e;
    const unsigned long long* a_k = o->f_ak[acur].as<unsigned long long>();
    const uint32_t *a_f = o->f_af[acur].as<uint32_t>(), *a_c = o->f_ac[acur].as<uint32_t>();
    MH_TRY(o->pk.reserve(n_e * 8));
    MH_TRY(o->pks.reserve(n_e * 8));
    MH_TRY(o->f_pf.reserve(n_e * 4));
    MH_TRY(o->f_pfs.reserve(n_e * 4));
    MH_TRY(o->head.reserve(n_e * 4));
    MH_TRY(o->pos.reserve(n_e * 4));
    MH_TRY(o->f_ek.reserve(n_e * 8));
    MH_TRY(o->f_ev.reserve(n_e * 8));
    unsigned long long *s_k = o->pks.as<unsigned long long>(), *s_k2 = o->pk.as<unsigned long long>();
    uint32_t *s_f = o->f_pf.as<uint32_t>(), *s_c = o->f_pfs.as<uint32_t>();
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, a_k, s_k, a_f, s_f, (size_t)n_e, 0, 64, s); }));
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, a_k, s_k2, a_c, s_c, (size_t)n_e, 0, 64, s); }));
    uint32_t *head = o->head.as<uint32_t>(), *pos = o->pos.as<uint32_t>();
    hipLaunchKernelGGL(k_occf_pair_heads, dim3(nblk(n_e, B)), dim3(B), 0, s, s_k, s_f, NE, head);
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, head, pos, 0u, (size_t)n_e, rocprim::plus<uint32_t>(), s);
    }));
    hipLaunchKernelGGL(k_occf_sum_runs, dim3(nblk(n_e, B)), dim3(B), 0, s, s_k, s_f, s_c, head, pos, NE,
                       o->f_ek.as<unsigned long long>(), o->f_ev.as<unsigned long long>());
    MH_HIP(hipGetLastError());
    o->h_rb[0] = o->h_rb[1] = 0;
    MH_HIP(hipMemcpyAsync(&o->h_rb[0], pos + (n_e - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(&o->h_rb[1], head + (n_e - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    n_e = (o->h_rb[0] & 0xFFFFFFFFull) + (o->h_rb[1] & 0xFFFFFFFFull);
    ek = o->f_ek.as<unsigned long long>();
    ev = o->f_ev.as<unsigned long long>();
  }
  // the call's totals take this pass in once it is complete: behind the swap of the store, or right here when it has nothing to fold
  auto pass_done = [&]() {
    o->n_left_out += left_out;
    o->n_keys += total;
    o->n_passes += n_chunks;
  };
  if (!n_e) {  // (every point of the pass was left out)
    pass_done();
    return MH_OK;
  }

  // ---- one slice of entries per touched cell
  const uint32_t NE = (uint32_t)n_e;
  MH_TRY(o->head.reserve(n_e * 4));
  MH_TRY(o->pos.reserve(n_e * 4));
  MH_TRY(o->ucell.reserve(n_e * 8 + 8));
  MH_TRY(o->f_ustart.reserve(n_e * 4 + 8));
  uint32_t *head = o->head.as<uint32_t>(), *pos = o->pos.as<uint32_t>();
  hipLaunchKernelGGL(k_occ_cell_heads, dim3(nblk(n_e, B)), dim3(B), 0, s, ek, NE, head);
  MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, head, pos, 0u, (size_t)n_e, rocprim::plus<uint32_t>(), s);
  }));
  hipLaunchKernelGGL(k_occf_cells, dim3(nblk(n_e, B)), dim3(B), 0, s, ek, head, pos, NE, o->ucell.as<unsigned long long>(),
                     o->f_ustart.as<uint32_t>());
  MH_HIP(hipGetLastError());
  o->h_rb[0] = o->h_rb[1] = 0;
  MH_HIP(hipMemcpyAsync(&o->h_rb[0], pos + (n_e - 1), 4, hipMemcpyDeviceToHost, s));
  MH_HIP(hipMemcpyAsync(&o->h_rb[1], head + (n_e - 1), 4, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  const uint64_t n_u = (o->h_rb[0] & 0xFFFFFFFFull) + (o->h_rb[1] & 0xFFFFFFFFull);

  // ---- the fold, the merge with the store, the occupied centres
  const uint64_t n_s = o->n_cells, n_t = n_s + n_u;
  MH_REQUIRE(n_t < 0x7FFFFFF0ull, "too many cells");
  const uint32_t NS = (uint32_t)n_s, NU = (uint32_t)n_u, NT = (uint32_t)n_t;
  const int nxt = o->cur ^ 1;
  MH_TRY(o->ulb.reserve(n_u * 4 + 4));
  MH_TRY(o->is_new.reserve((n_u + 1) * 4));
  MH_TRY(o->new_rank.reserve((n_u + 1) * 4));
  MH_TRY(o->f_unew.reserve(n_u * 4 + 4));
  MH_TRY(o->mkey.reserve(n_t * 8));
  MH_TRY(o->mlo.reserve(n_t * 4));
  MH_TRY(o->flags.reserve((n_t + 1) * 8));
  MH_TRY(o->fscan.reserve((n_t + 1) * 8));
  MH_TRY(o->skey[nxt].reserve(n_t * 8));
  MH_TRY(o->slo[nxt].reserve(n_t * 4));
  MH_TRY(o->cx.reserve(n_t * 4));
  MH_TRY(o->cy.reserve(n_t * 4));
  MH_TRY(o->cz.reserve(n_t * 4));
  const unsigned long long* skey = o->skey[o->cur].as<unsigned long long>();
  const int* slo = o->slo[o->cur].as<int>();
  uint32_t *is_new = o->is_new.as<uint32_t>(), *new_rank = o->new_rank.as<uint32_t>();
  hipLaunchKernelGGL(k_occf_fold, dim3(nblk(n_u + 1, B)), dim3(B), 0, s, o->ucell.as<unsigned long long>(), o->f_ustart.as<uint32_t>(),
                     NU, ek, ev, skey, slo, NS, o->rule, o->ulb.as<uint32_t>(), is_new, o->f_unew.as<int>());
  MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, is_new, new_rank, 0u, (size_t)n_u + 1, rocprim::plus<uint32_t>(), s);
  }));
  unsigned long long* flags = o->flags.as<unsigned long long>();
  unsigned long long* fscan = o->fscan.as<unsigned long long>();
  hipLaunchKernelGGL(k_occf_merge, dim3(nblk(n_t, B)), dim3(B), 0, s, skey, slo, NS, o->ucell.as<unsigned long long>(),
                     o->f_unew.as<int>(), o->ulb.as<uint32_t>(), is_new, new_rank, NU, o->rule.l_occ,
                     o->mkey.as<unsigned long long>(), o->mlo.as<int>(), flags);
  MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, flags, fscan, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), s);
  }));
  hipLaunchKernelGGL(k_occ_compact, dim3(nblk(n_t, B)), dim3(B), 0, s, o->mkey.as<unsigned long long>(), o->mlo.as<int>(), flags,
                     fscan, NT, PR.resolution, o->skey[nxt].as<unsigned long long>(), o->slo[nxt].as<int>(), o->cx.as<float>(),
                     o->cy.as<float>(), o->cz.as<float>());
  MH_HIP(hipGetLastError());
  MH_TRY(read_back(o, fscan + n_t, 1, s));
  o->n_cells = o->h_rb[0] >> 32;
  o->n_occupied = o->h_rb[0] & 0xFFFFFFFFull;
  o->cur = nxt;
  pass_done();
  return MH_OK;
}

}  // namespace

extern "C" {

uint32_t mh_occgrid_api_version(void) { return MH_OCCGRID_API_VERSION; }

mh_status mh_occmap_insert_frames(mh_occmap* o, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                  uint64_t max_points_per_pass) {
  MH_REQUIRE(o, "null map");
  uint64_t sum = 0;
  MH_TRY(frames_check(__func__, frames, n_frames, mem, &sum));  // (the refusals every batched posed-frame call shares)
  for (size_t f = 0; f < n_frames; f++)
    for (int a = 0; a < 3; a++)
      MH_REQUIRE(fabsf((float)frames[f].T[4 * a + 3] * o->inv_res) < 1.0e6f, "insertion pose outside the key range");
  if (sum == 0) return MH_OK;
  MH_REQUIRE(o->n_cells < 0x3FFFFFF0ull, "too many points");
  MH_TRY(set_device(o->ctx));
  o->n_left_out = o->n_keys = 0;
  o->n_passes = 0;
  const uint64_t budget = std::min<uint64_t>(max_points_per_pass ? max_points_per_pass : kFramesPassPoints, 0x7FFFFFEFull);
  const bool staged = mem != MH_MEM_DEVICE;
  const uint32_t dec = o->params.decimation;
  mh_status st = MH_OK;
  bool applied = false;
  size_t f0 = 0;
  while (f0 < n_frames && st == MH_OK) {
    uint64_t P = 0, S = 0;  // frames in order while they fit; a frame larger than the budget is a pass of its own
    const size_t f1 = frames_next_pass(frames, n_frames, f0, budget, &P);
    for (size_t f = f0; f < f1; f++) S += (frames[f].n + dec - 1) / dec;
    if (P == 0) break;  // (only empty frames were left)
    const int cur = o->cur;
    st = occ_frames_pass(o, frames + f0, f1 - f0, P, S, staged);
    applied = applied || o->cur != cur;
    f0 = f1;
  }
  if (st != MH_OK) (void)mh::wait_stream(o->ctx->stream);  // (nothing may still read the mirror or the caller's arrays)
  // the search map, once: over what the completed passes left, a failed call included
  if (applied) {
    const mh_status sr = inner_rebuild(o);
    if (st == MH_OK) st = sr;
  }
  return st;
}

mh_status mh_occmap_index_bounds(const mh_occmap* o, int32_t lo[3], int32_t hi[3], uint64_t* n_cells) {
  MH_REQUIRE(o && lo && hi && n_cells, "null argument");
  *n_cells = o->n_cells;
  if (!o->n_cells) return MH_OK;
  mh_occmap* w = const_cast<mh_occmap*>(o);  // (scratch and the read-back words are the handle's)
  MH_TRY(set_device(o->ctx));
  hipStream_t s = o->ctx->stream;
  MH_TRY(w->counters.reserve(256));
  int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  int got[6];
  MH_HIP(hipMemcpyAsync(w->counters.p, init, sizeof(init), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_occ_bounds, dim3(std::min<uint32_t>(nblk(o->n_cells, 256), 128u)), dim3(256), 0, s, o->skey[o->cur].as<unsigned long long>(),
                     (uint32_t)o->n_cells, w->counters.as<int>());
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(got, w->counters.p, sizeof(got), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  for (int a = 0; a < 3; a++) {
    lo[a] = got[a];
    hi[a] = got[3 + a];
  }
  return MH_OK;
}

mh_status mh_occmap_project_grid(const mh_occmap* o, const mh_occgrid_window* win, int32_t* max_logodds) {
  MH_REQUIRE(o && win && max_logodds, "null argument");
  MH_REQUIRE(win->nx > 0 && win->ny > 0, "nx and ny must be > 0");
  MH_REQUIRE((uint64_t)win->nx * (uint64_t)win->ny <= (1ull << 28), "nx * ny must not exceed 2^28");
  MH_REQUIRE(win->z_lo <= win->z_hi, "z_lo must not exceed z_hi");
  mh_occmap* w = const_cast<mh_occmap*>(o);
  MH_TRY(set_device(o->ctx));
  hipStream_t s = o->ctx->stream;
  const size_t n = (size_t)win->nx * win->ny;
  MH_TRY(w->f_grid.reserve(n * sizeof(int)));
  hipLaunchKernelGGL(k_occ_grid_fill, dim3(nblk(n, 256)), dim3(256), 0, s, w->f_grid.as<int>(), n, INT_MIN);
  if (o->n_cells)
    hipLaunchKernelGGL(k_occ_project, dim3(nblk(o->n_cells, 256)), dim3(256), 0, s, o->skey[o->cur].as<unsigned long long>(),
                       o->slo[o->cur].as<int>(), (uint32_t)o->n_cells, win->x0, win->y0, win->nx, win->ny, win->z_lo, win->z_hi,
                       w->f_grid.as<int>());
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(max_logodds, w->f_grid.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
