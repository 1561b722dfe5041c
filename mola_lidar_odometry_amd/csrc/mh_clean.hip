// mh_clean.hip -- see-through voting on key-frame views: the store of views mh_views, mh_views_add_frames and
// mh_views_vote_frames (kernels in mh_k_clean.h; the specification is the text of include/molahip_clean.h).  A translation unit
// of its own: nothing here touches a map.
//
// add_frames:  per pass of frames one upload through a page-locked mirror [points | prefix array | frame table], the new views
//              preset to "empty", one flat k_view_build over all points of the pass straight into the store.
// vote_frames: the neighbour list up once; per pass the same upload plus the tile prefix array, one k_see_through (one workgroup
//              per frame and tile), the packed words out.
// Scratch is the context's grow-only buffers (staging, compact); everything is ordered on the context's stream and every call
// blocks until its output is where the caller asked for it.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "molahip_clean.h"
#include "mh_internal.h"
#include "mh_views.h"
#include "mh_k_clean.h"

using namespace mh;

namespace {

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
inline bool mem_ok(int32_t mem) { return mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED; }

constexpr uint64_t kCleanPassPoints = 1ull << 21;  // 24 MB of staged coordinates

// the host tables of the specification: fp64, rounded once to fp32.  False: parameters outside the specified ranges.
bool clean_make_tables(const mh_clean_params* p, CleanTables& t) {
  if (!p) return false;
  if (p->n_rings < 1 || p->n_rings > MH_CLEAN_MAX_RINGS) return false;
  if (p->n_sectors < 8 || p->n_sectors > MH_CLEAN_MAX_SECTORS || p->n_sectors % 8) return false;
  if ((uint64_t)p->n_rings * p->n_sectors > MH_CLEAN_MAX_BINS) return false;
  if (p->win_rings > 2 || p->win_sectors > 2) return false;
  const float v[] = {p->el_min, p->el_max, p->min_range, p->max_range, p->rel_margin, p->origin[0], p->origin[1], p->origin[2]};
  for (float f : v)
    if (!isfinite(f)) return false;
  const double half_pi = 1.57079632679489661923;
  if (!((double)p->el_min > -half_pi && p->el_min < p->el_max && (double)p->el_max < half_pi)) return false;
  if (!(p->min_range > 0.f && p->min_range < p->max_range && p->rel_margin > 0.f)) return false;
  memset(&t, 0, sizeof(t));
  t.A = p->n_rings;
  t.S = p->n_sectors;
  t.win_rings = p->win_rings;
  t.win_sectors = p->win_sectors;
  for (uint32_t j = 1; j < t.S / 8; j++) t.tan_edge[j] = (float)tan(2.0 * 3.14159265358979323846 * (double)j / (double)t.S);
  const double e0 = (double)p->el_min, de = (double)p->el_max - (double)p->el_min;
  for (uint32_t k = 0; k <= t.A; k++) {
    const double e = e0 + (double)k * de / (double)t.A;
    const double tn = tan(e);
    t.el_tan2[k] = (float)(tn * tn);
    t.el_sign[k] = e > 0.0 ? 1 : (e < 0.0 ? -1 : 0);
    if (!isfinite(t.el_tan2[k])) return false;
  }
  t.min_r2 = (float)((double)p->min_range * (double)p->min_range);
  t.max_r2 = (float)((double)p->max_range * (double)p->max_range);
  const double m = 1.0 + (double)p->rel_margin;
  t.far2 = (float)(m * m);
  t.ox = p->origin[0]; t.oy = p->origin[1]; t.oz = p->origin[2];
  return t.min_r2 > 0.f && isfinite(t.max_r2) && isfinite(t.far2);
}

mh_status frames_ok(const char* fn, const mh_map_frame* frames, size_t n_frames) {
  if (n_frames && !frames) return fail(MH_ERR_INVALID_ARGUMENT, "%s: null frames", fn);
  for (size_t f = 0; f < n_frames; f++) {
    if (frames[f].n && !(frames[f].x && frames[f].y && frames[f].z)) return fail(MH_ERR_INVALID_ARGUMENT, "%s: null point arrays", fn);
    if (frames[f].n >= 0x7FFFFFF0ull) return fail(MH_ERR_INVALID_ARGUMENT, "%s: too many points", fn);
  }
  return MH_OK;
}

// One pass of frames [f0, f1) as uploaded: [x | y | z of the pass's points (host arrays only)] | point prefix array [nf + 1] |
// tile prefix array [nf + 1] | frame table [nf]
struct Pass {
  size_t f1 = 0, nf = 0;
  uint64_t P = 0;         // points
  uint32_t n_tiles = 0;   // tiles of kCleanBlock points, per frame
  const uint32_t *d_start = nullptr, *d_tiles = nullptr;
  const PlaceSrc* d_table = nullptr;
};

// packs the pass that begins at f0 into the mirror and starts its one upload on the context's stream
mh_status stage_pass(mh_ctx* ctx, PinnedBuf& mirror, const mh_map_frame* frames, size_t n_frames, size_t f0, int32_t mem,
                     uint64_t budget, Pass& ps) {
  hipStream_t s = ctx->stream;
  const bool staged = mem != MH_MEM_DEVICE;  // host arrays travel through the mirror; device arrays are read in place
  size_t f1 = f0;
  uint64_t P = 0;  // frames in order while they fit; a frame larger than the budget is a pass of its own
  while (f1 < n_frames && (f1 == f0 || P + frames[f1].n <= budget)) P += frames[f1++].n;
  const size_t nf = f1 - f0;
  const size_t pstride = staged ? up256(P * sizeof(float)) : 0;
  const size_t off_start = 3 * pstride;
  const size_t off_tiles = off_start + up256((nf + 1) * sizeof(uint32_t));
  const size_t off_table = off_tiles + up256((nf + 1) * sizeof(uint32_t));
  const size_t up_bytes = off_table + nf * sizeof(PlaceSrc);
  MH_HIP(mh::wait_stream(s));  // the previous pass has read the mirror
  MH_TRY(mirror.reserve(up_bytes));
  MH_TRY(ctx->staging.reserve(up_bytes));
  char* h = mirror.as<char>();
  char* d = ctx->staging.as<char>();
  uint32_t* h_start = (uint32_t*)(h + off_start);
  uint32_t* h_tiles = (uint32_t*)(h + off_tiles);
  PlaceSrc* h_tab = (PlaceSrc*)(h + off_table);
  uint64_t at = 0, tiles = 0;
  for (size_t k = 0; k < nf; k++) {
    const mh_map_frame& fr = frames[f0 + k];
    h_start[k] = (uint32_t)at;
    h_tiles[k] = (uint32_t)tiles;
    PlaceSrc& e = h_tab[k];
    if (staged) {
      if (fr.n) {
        memcpy(h + at * sizeof(float), fr.x, fr.n * sizeof(float));
        memcpy(h + pstride + at * sizeof(float), fr.y, fr.n * sizeof(float));
        memcpy(h + 2 * pstride + at * sizeof(float), fr.z, fr.n * sizeof(float));
      }
      e.x = (const float*)d + at;
      e.y = (const float*)(d + pstride) + at;
      e.z = (const float*)(d + 2 * pstride) + at;
    } else {
      e.x = fr.x; e.y = fr.y; e.z = fr.z;
    }
    at += fr.n;
    tiles += (fr.n + kCleanBlock - 1) / kCleanBlock;
  }
  h_start[nf] = (uint32_t)at;
  h_tiles[nf] = (uint32_t)tiles;
  MH_HIP(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s));  // the pass's one upload
  ps.f1 = f1; ps.nf = nf; ps.P = P; ps.n_tiles = (uint32_t)tiles;
  ps.d_start = (const uint32_t*)(d + off_start);
  ps.d_tiles = (const uint32_t*)(d + off_tiles);
  ps.d_table = (const PlaceSrc*)(d + off_table);
  return MH_OK;
}

}  // namespace

extern "C" {

uint32_t mh_clean_api_version(void) { return MH_CLEAN_API_VERSION; }

mh_status mh_views_create(mh_ctx* ctx, const mh_clean_params* params, mh_views** out) {
  MH_REQUIRE(ctx && params && out, "null argument");
  *out = nullptr;
  CleanTables tab;
  MH_REQUIRE(clean_make_tables(params, tab), "cleaning parameters outside their ranges");
  mh_views* v = new (std::nothrow) mh_views();
  if (!v) return fail(MH_ERR_OUT_OF_MEMORY, "host allocation failed");
  v->ctx = ctx;
  v->params = *params;
  v->tab = tab;
  *out = v;
  return MH_OK;
}

mh_status mh_views_destroy(mh_views* v) {
  if (!v) return MH_OK;
  (void)set_device(v->ctx);
  (void)mh::wait_stream(v->ctx->stream);
  v->img.release();
  v->nbr.release();
  v->h_frames.release();
  delete v;
  return MH_OK;
}

mh_status mh_views_size(const mh_views* v, uint64_t* n) {
  MH_REQUIRE(v && n, "null argument");
  *n = v->size;
  return MH_OK;
}

mh_status mh_views_add_frames(mh_views* v, const mh_map_frame* frames, size_t n_frames, int32_t mem, uint64_t max_points_per_pass) {
  MH_REQUIRE(v, "null views");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  MH_TRY(frames_ok(__func__, frames, n_frames));
  MH_REQUIRE(v->size + n_frames < 0xFFFFFFF0ull, "too many views");
  if (n_frames == 0) return MH_OK;
  mh_ctx* ctx = v->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t AS = (size_t)v->tab.A * v->tab.S;
  const uint64_t budget = max_points_per_pass ? max_points_per_pass : kCleanPassPoints;
  MH_TRY(views_reserve(v, v->size + n_frames));
  MH_HIP(hipMemsetAsync(v->img.as<uint32_t>() + v->size * AS, 0xFF, n_frames * AS * sizeof(uint32_t), s));  // all empty
  size_t f0 = 0;
  while (f0 < n_frames) {
    Pass ps;
    MH_TRY(stage_pass(ctx, v->h_frames, frames, n_frames, f0, mem, budget, ps));
    if (ps.P) {
      hipLaunchKernelGGL(k_view_build, dim3(nblk(ps.P, kPlaceChunk)), dim3(kPlaceBlock), 0, s, ps.d_start, ps.d_table, (uint32_t)ps.nf,
                         (uint32_t)ps.P, v->tab, v->img.as<uint32_t>() + (v->size + f0) * AS);
      MH_HIP(hipGetLastError());
    }
    f0 = ps.f1;
  }
  MH_HIP(mh::wait_stream(s));  // the caller's arrays may be reused; the views are stored
  v->size += n_frames;
  return MH_OK;
}

mh_status mh_views_download(const mh_views* v, uint64_t first, uint64_t n, uint32_t* out) {
  MH_REQUIRE(v, "null views");
  MH_REQUIRE(first <= v->size && n <= v->size - first, "range beyond the store");
  MH_REQUIRE(out || n == 0, "null output");
  if (n == 0) return MH_OK;
  MH_TRY(set_device(v->ctx));
  const size_t AS = (size_t)v->tab.A * v->tab.S;
  MH_HIP(hipMemcpyAsync(out, v->img.as<uint32_t>() + first * AS, n * AS * sizeof(uint32_t), hipMemcpyDeviceToHost, v->ctx->stream));
  MH_HIP(mh::wait_stream(v->ctx->stream));
  return MH_OK;
}

mh_status mh_views_vote_frames(const mh_views* cv, const mh_map_frame* frames, size_t n_frames, const uint32_t* nbr_start,
                               const uint32_t* nbr_view, const double* nbr_T, uint32_t* votes_out, int32_t mem,
                               uint64_t max_points_per_pass) {
  mh_views* v = const_cast<mh_views*>(cv);  // (the stored views are read only; the mirror and the list buffer are scratch)
  MH_REQUIRE(v, "null views");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  MH_TRY(frames_ok(__func__, frames, n_frames));
  if (n_frames == 0) return MH_OK;
  MH_REQUIRE(nbr_start, "null neighbour offsets");
  MH_REQUIRE(n_frames < 0xFFFFFFF0ull, "too many frames");
  uint64_t total = 0;
  for (size_t f = 0; f < n_frames; f++) {
    MH_REQUIRE(nbr_start[f] <= nbr_start[f + 1], "nbr_start is not non-decreasing");
    total += frames[f].n;
  }
  MH_REQUIRE(votes_out || total == 0, "null votes_out");
  const uint32_t k0 = nbr_start[0], k1 = nbr_start[n_frames];
  MH_REQUIRE(k0 == k1 || (nbr_view && nbr_T), "null neighbour list");
  for (uint32_t k = k0; k < k1; k++) {
    MH_REQUIRE(nbr_view[k] < v->size, "neighbour index beyond the store");
    for (int e = 0; e < 12; e++) MH_REQUIRE(isfinite(nbr_T[12 * (size_t)k + e]), "non-finite pose entry");
  }
  if (total == 0) return MH_OK;
  mh_ctx* ctx = v->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const bool to_device = mem == MH_MEM_DEVICE;
  const uint64_t budget = max_points_per_pass ? max_points_per_pass : kCleanPassPoints;
  // the neighbour list: offsets [n_frames + 1] | view indices [k1] | poses [12 * k1]  (indexed as the caller indexes them)
  const size_t off_view = up256((n_frames + 1) * sizeof(uint32_t));
  const size_t off_T = off_view + up256((size_t)k1 * sizeof(uint32_t));
  MH_TRY(v->nbr.reserve(off_T + (size_t)k1 * 12 * sizeof(double) + 8));
  char* dn = v->nbr.as<char>();
  MH_HIP(hipMemcpyAsync(dn, nbr_start, (n_frames + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (k1 > k0) {
    MH_HIP(hipMemcpyAsync(dn + off_view + (size_t)k0 * sizeof(uint32_t), nbr_view + k0, (size_t)(k1 - k0) * sizeof(uint32_t),
                          hipMemcpyHostToDevice, s));
    MH_HIP(hipMemcpyAsync(dn + off_T + (size_t)k0 * 12 * sizeof(double), nbr_T + 12 * (size_t)k0,
                          (size_t)(k1 - k0) * 12 * sizeof(double), hipMemcpyHostToDevice, s));
  }
  MH_HIP(mh::wait_stream(s));  // (pageable sources: the caller's list may be reused)
  size_t f0 = 0;
  uint64_t done = 0;
  while (f0 < n_frames) {
    Pass ps;
    MH_TRY(stage_pass(ctx, v->h_frames, frames, n_frames, f0, mem, budget, ps));
    if (ps.P) {
      if (!to_device) MH_TRY(ctx->compact.reserve(ps.P * sizeof(uint32_t)));
      uint32_t* d_votes = to_device ? votes_out + done : ctx->compact.as<uint32_t>();
      hipLaunchKernelGGL(k_see_through, dim3(ps.n_tiles), dim3(kCleanBlock), 0, s, ps.d_tiles, ps.d_start, ps.d_table, (uint32_t)ps.nf,
                         (const uint32_t*)dn + f0, (const uint32_t*)(dn + off_view), (const double*)(dn + off_T),
                         (const uint32_t*)v->img.as<uint32_t>(), v->tab, d_votes);
      MH_HIP(hipGetLastError());
      if (!to_device) MH_HIP(hipMemcpyAsync(votes_out + done, d_votes, ps.P * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    done += ps.P;
    f0 = ps.f1;
  }
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
