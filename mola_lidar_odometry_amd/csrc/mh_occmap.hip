// mh_occmap.hip -- device-resident occupancy voxel map: the stand-in for mrpt::maps::CVoxelMap [U] (lidar2d.yaml:183-198)
// in its two roles for the odometry pipeline: the ray-traced log-odds update of a key-frame, and the NN-search target made of
// the centres of its occupied voxels.  The reading implemented is written down at mh_occmap_insert in include/molahip.h.
//
// The store is two sorted arrays (keys ascending, log-odds), nothing looks a cell up except the merge.  An insert writes one
// 64-bit key per (ray, step) and per end cell (mh_k_occ.h), sorts them (rocPRIM, like mh_map.hip), run-length encodes them
// into per-cell hit / miss counts, merge-joins those with the store, applies the update rule once per cell, removes far
// cells, and rebuilds the inner mh_map from the occupied centres.  Every step is independent of thread order.
#include <math.h>

#include <algorithm>
#include <new>
#include <vector>

#include "mh_occmap_internal.h"

using namespace mh;
using namespace mh::occ;

namespace {

// log-odds of a probability, scale 16
double lo16(double p) { return 16.0 * log(p / (1.0 - p)); }
bool in01(float p) { return p > 0.f && p < 1.f; }

}  // namespace

extern "C" {

mh_status mh_occmap_create(mh_ctx* ctx, const mh_occmap_params* p, mh_occmap** out) {
  MH_REQUIRE(p && out, "null argument");
  *out = nullptr;
  MH_REQUIRE(p->resolution > 0.f && isfinite(p->resolution), "resolution must be > 0");
  MH_REQUIRE(in01(p->prob_hit) && in01(p->prob_miss), "prob_hit and prob_miss must lie inside (0, 1)");
  MH_REQUIRE(in01(p->clamp_min) && in01(p->clamp_max), "clamp_min and clamp_max must lie inside (0, 1)");
  MH_REQUIRE(p->clamp_min < p->clamp_max, "clamp_min must be below clamp_max");
  MH_REQUIRE(in01(p->occupied_threshold), "occupied_threshold must lie inside (0, 1)");
  MH_REQUIRE(p->decimation >= 1, "decimation must be >= 1");
  MH_REQUIRE(p->update_rule == MH_OCC_COUNTED || p->update_rule == MH_OCC_ONCE, "unknown update_rule");
  MH_REQUIRE(p->index_mode == MH_INDEX_FLOOR || p->index_mode == MH_INDEX_TRUNC, "bad index_mode");
  MH_REQUIRE(p->far_voxel_metric <= MH_FAR_L2, "bad far_voxel_metric");
  MH_REQUIRE(p->max_range >= 0.f, "negative max_range");
  MH_REQUIRE(p->search_voxel_size >= 0.f && isfinite(p->search_voxel_size), "negative search_voxel_size");
  MH_REQUIRE(ctx, "null argument");
  mh_occmap* o = new (std::nothrow) mh_occmap();
  if (!o) return fail(MH_ERR_OUT_OF_MEMORY, "host allocation failed");
  o->ctx = ctx;
  o->params = *p;
  o->inv_res = 1.0f / p->resolution;
  // the five integers, once, in double: the device only ever sees these
  o->rule.l_hit = std::max(1, (int)floor(lo16((double)p->prob_hit) + 0.5));
  o->rule.l_miss = std::max(1, (int)floor(-lo16((double)p->prob_miss) + 0.5));
  o->rule.l_min = (int)floor(lo16((double)p->clamp_min) + 0.5);
  o->rule.l_max = (int)floor(lo16((double)p->clamp_max) + 0.5);
  o->rule.l_occ = (int)floor(lo16((double)p->occupied_threshold)) + 1;
  o->rule.once = p->update_rule == MH_OCC_ONCE;
  o->max_keys_per_pass = p->max_keys_per_pass ? p->max_keys_per_pass : kDefaultKeysPerPass;
  if (o->max_keys_per_pass > 0x7FFFFFF0ull) o->max_keys_per_pass = 0x7FFFFFF0ull;
  const float v0 = p->search_voxel_size > 0.f ? p->search_voxel_size : 1.0f;
  mh_status st = set_device(ctx);
  if (st == MH_OK && hipHostMalloc((void**)&o->h_rb, 4 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
    st = fail(MH_ERR_OUT_OF_MEMORY, "pinned allocation failed");
  if (st == MH_OK) st = inner_replace(o, v0);
  if (st != MH_OK) {
    if (o->h_rb) (void)hipHostFree(o->h_rb);
    delete o;
    return st;
  }
  *out = o;
  return MH_OK;
}

mh_status mh_occmap_destroy(mh_occmap* o) {
  if (!o) return MH_OK;
  (void)hipSetDevice(o->ctx->device);
  (void)mh::wait_stream(o->ctx->stream);
  (void)mh_map_destroy(o->inner);
  if (o->h_rb) (void)hipHostFree(o->h_rb);
  for (DevBuf* b : {&o->skey[0], &o->skey[1], &o->slo[0], &o->slo[1], &o->cx, &o->cy, &o->cz, &o->ray_e, &o->items, &o->prefix,
                    &o->counters, &o->pk, &o->pks, &o->rk, &o->rc, &o->ak[0], &o->ak[1], &o->ac[0], &o->ac[1], &o->mk, &o->mc,
                    &o->head, &o->pos, &o->ucell, &o->uh, &o->um, &o->ulb, &o->is_new, &o->new_rank, &o->mkey, &o->mlo,
                    &o->flags, &o->fscan, &o->tmp, &o->f_up, &o->f_rayf, &o->f_pf, &o->f_pfs, &o->f_ek, &o->f_ev, &o->f_ak[0],
                    &o->f_ak[1], &o->f_af[0], &o->f_af[1], &o->f_ac[0], &o->f_ac[1], &o->f_ustart, &o->f_unew, &o->f_grid})
    b->release();
  o->f_h.release();
  delete o;
  return MH_OK;
}

mh_status mh_occmap_clear(mh_occmap* o) {
  MH_REQUIRE(o, "null argument");
  MH_TRY(set_device(o->ctx));
  MH_HIP(mh::wait_stream(o->ctx->stream));
  o->n_cells = o->n_occupied = 0;
  o->n_left_out = o->n_keys = 0;
  o->n_passes = 0;
  const float v0 = o->params.search_voxel_size > 0.f ? o->params.search_voxel_size : 1.0f;
  if (o->V != v0) return inner_replace(o, v0);  // a cleared map behaves as a new one: the search voxel starts over
  return inner_rebuild(o);
}

mh_status mh_occmap_insert(mh_occmap* o, const mh_scan* scan, const double T[12], float remove_voxels_farther_than) {
  MH_REQUIRE(o && scan && T, "null argument");
  MH_REQUIRE(o->ctx == scan->ctx, "map and scan belong to different contexts");
  MH_REQUIRE(remove_voxels_farther_than >= 0.f, "negative remove_voxels_farther_than");
  for (int i = 0; i < 12; i++) MH_REQUIRE(isfinite(T[i]), "non-finite pose");
  const mh_occmap_params& P = o->params;
  const bool trunc = P.index_mode == MH_INDEX_TRUNC;
  int oc[3];
  for (int a = 0; a < 3; a++) {  // the cell of the pose's translation: ray origin and centre of the far removal
    const float sc = (float)T[4 * a + 3] * o->inv_res;
    MH_REQUIRE(fabsf(sc) < 1.0e6f, "insertion pose outside the key range");
    oc[a] = trunc ? (int)sc : (int)floorf(sc);
  }
  const size_t n_sel = (scan->n + P.decimation - 1) / P.decimation;
  MH_REQUIRE(n_sel < 0x7FFFFFF0ull && o->n_cells < 0x3FFFFFF0ull, "too many points");
  mh_ctx* ctx = o->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const uint32_t B = 256;
  o->n_left_out = o->n_keys = 0;
  o->n_passes = 0;

  // ---- rays: end cells, work items, their prefix sum
  uint64_t total = 0;
  if (n_sel) {
    const uint32_t N = (uint32_t)n_sel;
    MH_TRY(o->ray_e.reserve(n_sel * sizeof(int4)));
    MH_TRY(o->items.reserve(n_sel * sizeof(uint32_t)));
    MH_TRY(o->prefix.reserve((n_sel + 1) * sizeof(unsigned long long)));
    MH_TRY(o->counters.reserve(256));
    MH_HIP(hipMemsetAsync(o->counters.p, 0, 256, s));
    Pose12 P12;
    for (int i = 0; i < 12; i++) P12.m[i] = T[i];
    hipLaunchKernelGGL(k_occ_rays, dim3(nblk(n_sel, B)), dim3(B), 0, s, scan->x, scan->y, scan->z, N, P.decimation, P12, (float)T[3],
                       (float)T[7], (float)T[11], oc[0], oc[1], oc[2], o->inv_res, (uint32_t)trunc,
                       P.max_range > 0.f ? P.max_range * P.max_range : -1.f, P.ray_trace_free_space ? 1u : 0u, o->ray_e.as<int4>(),
                       o->items.as<uint32_t>(), o->counters.as<uint32_t>());
    MH_HIP(hipGetLastError());
    auto in = rocprim::make_transform_iterator(o->items.as<uint32_t>(), ToU64());
    unsigned long long* prefix = o->prefix.as<unsigned long long>();
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, in, prefix, 0ull, n_sel, rocprim::plus<unsigned long long>(), s);
    }));
    // total = prefix[last] + items[last]; the left-out counter rides along
    o->h_rb[1] = o->h_rb[2] = 0;
    MH_HIP(hipMemcpyAsync(&o->h_rb[0], prefix + (n_sel - 1), 8, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(&o->h_rb[1], o->items.as<uint32_t>() + (n_sel - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(&o->h_rb[2], o->counters.p, 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    total = o->h_rb[0] + (o->h_rb[1] & 0xFFFFFFFFull);
    o->n_left_out = o->h_rb[2] & 0xFFFFFFFFull;
  }
  o->n_keys = total;

  // ---- keys, in passes of at most max_keys_per_pass: sorted, run-length encoded, summed by key into the accumulated entries
  int acur = 0;
  uint64_t n_acc = 0;
  const unsigned long long* ek = nullptr;  // the (cell << 1 | is_miss, count) entries of the whole insert
  const uint32_t* ec = nullptr;
  for (uint64_t g0 = 0; g0 < total; g0 += o->max_keys_per_pass) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(o->max_keys_per_pass, total - g0);
    o->n_passes++;
    MH_TRY(o->pk.reserve((size_t)cnt * 8));
    MH_TRY(o->pks.reserve((size_t)cnt * 8));
    MH_TRY(o->rk.reserve((size_t)cnt * 8));
    MH_TRY(o->rc.reserve((size_t)cnt * 4 + 8));
    unsigned long long *pk = o->pk.as<unsigned long long>(), *pks = o->pks.as<unsigned long long>();
    unsigned long long* rk = o->rk.as<unsigned long long>();
    uint32_t* rc = o->rc.as<uint32_t>();
    uint32_t* d_runs = rc + cnt;
    hipLaunchKernelGGL(k_occ_keys, dim3(nblk(cnt, B)), dim3(B), 0, s, o->prefix.as<unsigned long long>(), o->ray_e.as<int4>(),
                       (uint32_t)n_sel, oc[0], oc[1], oc[2], P.ray_trace_free_space ? 1u : 0u, (unsigned long long)g0, cnt, pk);
    MH_HIP(hipGetLastError());
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, pk, pks, (size_t)cnt, 0, 64, s); }));
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) { return rocprim::run_length_encode(t, b, pks, (size_t)cnt, rk, rc, d_runs, s); }));
    o->h_rb[0] = 0;
    MH_HIP(hipMemcpyAsync(&o->h_rb[0], d_runs, 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    const uint64_t n_runs = o->h_rb[0] & 0xFFFFFFFFull;
    if (n_acc == 0 && g0 + cnt >= total) {  // the only pass: its runs are the entries
      ek = rk;
      ec = rc;
      n_acc = n_runs;
      break;
    }
    if (n_acc == 0) {
      MH_TRY(o->ak[acur].reserve(n_runs * 8));
      MH_TRY(o->ac[acur].reserve(n_runs * 4));
      MH_HIP(hipMemcpyAsync(o->ak[acur].p, rk, n_runs * 8, hipMemcpyDeviceToDevice, s));
      MH_HIP(hipMemcpyAsync(o->ac[acur].p, rc, n_runs * 4, hipMemcpyDeviceToDevice, s));
      n_acc = n_runs;
    } else {  // merge the pass's runs into the accumulated entries and sum equal keys
      const uint64_t n_m = n_acc + n_runs;
      MH_TRY(o->mk.reserve(n_m * 8));
      MH_TRY(o->mc.reserve(n_m * 4));
      MH_TRY(o->ak[acur ^ 1].reserve(n_m * 8));
      MH_TRY(o->ac[acur ^ 1].reserve(n_m * 4 + 8));
      unsigned long long* mk = o->mk.as<unsigned long long>();
      uint32_t* mc = o->mc.as<uint32_t>();
      unsigned long long* a_k = o->ak[acur].as<unsigned long long>();
      uint32_t* a_c = o->ac[acur].as<uint32_t>();
      unsigned long long* n_k = o->ak[acur ^ 1].as<unsigned long long>();
      uint32_t* n_c = o->ac[acur ^ 1].as<uint32_t>();
      uint32_t* d_n = n_c + n_m;
      MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
        return rocprim::merge(t, b, a_k, rk, mk, a_c, rc, mc, (size_t)n_acc, (size_t)n_runs, rocprim::less<unsigned long long>(), s);
      }));
      MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
        return rocprim::reduce_by_key(t, b, mk, mc, (size_t)n_m, n_k, n_c, d_n, rocprim::plus<uint32_t>(),
                                      rocprim::equal_to<unsigned long long>(), s);
      }));
      o->h_rb[0] = 0;
      MH_HIP(hipMemcpyAsync(&o->h_rb[0], d_n, 4, hipMemcpyDeviceToHost, s));
      MH_HIP(mh::wait_stream(s));
      n_acc = o->h_rb[0] & 0xFFFFFFFFull;
      acur ^= 1;
    }
    ek = o->ak[acur].as<unsigned long long>();
    ec = o->ac[acur].as<uint32_t>();
  }

  // ---- one (cell, h, m) entry per touched cell
  uint64_t n_u = 0;
  MH_TRY(o->is_new.reserve((n_acc + 1) * 4));
  MH_TRY(o->new_rank.reserve((n_acc + 1) * 4));
  MH_TRY(o->ucell.reserve(n_acc * 8 + 8));
  MH_TRY(o->uh.reserve(n_acc * 4 + 4));
  MH_TRY(o->um.reserve(n_acc * 4 + 4));
  MH_TRY(o->ulb.reserve(n_acc * 4 + 4));
  if (n_acc) {
    const uint32_t NA = (uint32_t)n_acc;
    MH_TRY(o->head.reserve(n_acc * 4));
    MH_TRY(o->pos.reserve(n_acc * 4));
    uint32_t *head = o->head.as<uint32_t>(), *pos = o->pos.as<uint32_t>();
    hipLaunchKernelGGL(k_occ_cell_heads, dim3(nblk(n_acc, B)), dim3(B), 0, s, ek, NA, head);
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, head, pos, 0u, (size_t)n_acc, rocprim::plus<uint32_t>(), s);
    }));
    hipLaunchKernelGGL(k_occ_cells, dim3(nblk(n_acc, B)), dim3(B), 0, s, ek, ec, head, pos, NA, o->ucell.as<unsigned long long>(),
                       o->uh.as<uint32_t>(), o->um.as<uint32_t>());
    MH_HIP(hipGetLastError());
    o->h_rb[0] = o->h_rb[1] = 0;
    MH_HIP(hipMemcpyAsync(&o->h_rb[0], pos + (n_acc - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(&o->h_rb[1], head + (n_acc - 1), 4, hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));
    n_u = (o->h_rb[0] & 0xFFFFFFFFull) + (o->h_rb[1] & 0xFFFFFFFFull);
  }

  // ---- merge-join with the store, the rule, far removal, the occupied centres
  const uint64_t n_s = o->n_cells, n_t = n_s + n_u;
  MH_REQUIRE(n_t < 0x7FFFFFF0ull, "too many cells");
  if (n_t) {
    const uint32_t NS = (uint32_t)n_s, NU = (uint32_t)n_u, NT = (uint32_t)n_t;
    const int nxt = o->cur ^ 1;
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
    hipLaunchKernelGGL(k_occ_join, dim3(nblk(n_u + 1, B)), dim3(B), 0, s, o->ucell.as<unsigned long long>(), NU, skey, NS,
                       o->ulb.as<uint32_t>(), is_new);
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, is_new, new_rank, 0u, (size_t)n_u + 1, rocprim::plus<uint32_t>(), s);
    }));
    int4 ev = make_int4(0, 0, 0, -1);
    if (remove_voxels_farther_than > 0.f)
      ev = make_int4(oc[0], oc[1], oc[2], (int)ceilf(remove_voxels_farther_than * o->inv_res));
    unsigned long long* flags = o->flags.as<unsigned long long>();
    unsigned long long* fscan = o->fscan.as<unsigned long long>();
    hipLaunchKernelGGL(k_occ_merge, dim3(nblk(n_t, B)), dim3(B), 0, s, skey, slo, NS, o->ucell.as<unsigned long long>(),
                       o->uh.as<uint32_t>(), o->um.as<uint32_t>(), o->ulb.as<uint32_t>(), is_new, new_rank, NU, o->rule, ev,
                       P.far_voxel_metric, o->mkey.as<unsigned long long>(), o->mlo.as<int>(), flags);
    MH_TRY(with_tmp(o, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, flags, fscan, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), s);
    }));
    hipLaunchKernelGGL(k_occ_compact, dim3(nblk(n_t, B)), dim3(B), 0, s, o->mkey.as<unsigned long long>(), o->mlo.as<int>(), flags,
                       fscan, NT, P.resolution, o->skey[nxt].as<unsigned long long>(), o->slo[nxt].as<int>(), o->cx.as<float>(),
                       o->cy.as<float>(), o->cz.as<float>());
    MH_HIP(hipGetLastError());
    MH_TRY(read_back(o, fscan + n_t, 1, s));
    o->n_cells = o->h_rb[0] >> 32;
    o->n_occupied = o->h_rb[0] & 0xFFFFFFFFull;
    o->cur = nxt;
  }
  return inner_rebuild(o);
}

mh_status mh_occmap_get_info(const mh_occmap* o, mh_occmap_info* info) {
  MH_REQUIRE(o && info, "null argument");
  info->n_cells = o->n_cells;
  info->n_occupied = o->n_occupied;
  info->l_hit = o->rule.l_hit;
  info->l_miss = o->rule.l_miss;
  info->l_min = o->rule.l_min;
  info->l_max = o->rule.l_max;
  info->l_occ = o->rule.l_occ;
  info->search_voxel_size = o->V;
  info->n_left_out = o->n_left_out;
  info->n_keys = o->n_keys;
  info->n_passes = o->n_passes;
  info->reserved_ = 0;
  return MH_OK;
}

mh_status mh_occmap_download(const mh_occmap* o, int32_t* keys_xyz, int32_t* logodds) {
  MH_REQUIRE(o, "null argument");
  MH_TRY(set_device(o->ctx));
  MH_HIP(mh::wait_stream(o->ctx->stream));
  if (!o->n_cells) return MH_OK;
  if (keys_xyz) {
    std::vector<unsigned long long> k(o->n_cells);
    MH_HIP(hipMemcpy(k.data(), o->skey[o->cur].p, o->n_cells * 8, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < o->n_cells; v++) {
      int kx, ky, kz;
      unpack_key(k[v], kx, ky, kz);
      keys_xyz[3 * v] = kx;
      keys_xyz[3 * v + 1] = ky;
      keys_xyz[3 * v + 2] = kz;
    }
  }
  if (logodds) MH_HIP(hipMemcpy(logodds, o->slo[o->cur].p, o->n_cells * 4, hipMemcpyDeviceToHost));
  return MH_OK;
}

mh_status mh_occmap_search_map(mh_occmap* o, float min_radius, const mh_map** out) {
  MH_REQUIRE(o && out, "null argument");
  *out = nullptr;
  MH_REQUIRE(min_radius >= 0.f && isfinite(min_radius), "min_radius must be finite and >= 0");
  float v = o->V;
  while (v < min_radius) v *= 2.f;
  if (v != o->V) {  // the 27-voxel search is exact up to the voxel size: rebuild once with a voxel that suffices
    MH_TRY(set_device(o->ctx));
    MH_HIP(mh::wait_stream(o->ctx->stream));
    MH_TRY(inner_replace(o, v));
  }
  *out = o->inner;
  return MH_OK;
}

}  // extern "C"
