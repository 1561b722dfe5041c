// mh_place.hip -- place recognition by a polar height descriptor: mh_place_describe, the descriptor database mh_place_db and
// mh_place_search (kernels in mh_k_place.h; the specification is at the entry points in include/molahip.h).  A translation
// unit of its own: nothing here touches a map.
//
// describe:    [start | frame table] up -> zero the 32-bit bins -> k_place_describe -> k_place_pack -> bytes out.
// add_frames:  the same per pass of frames (one upload through a page-locked mirror, one flat launch over all points of the
//              pass), the pack pass writing straight behind the stored descriptors.
// search:      query up -> k_place_search over every stored descriptor -> matches out.
// Scratch is the context's grow-only buffers (staging, compact); everything is ordered on the context's stream and every call
// blocks until its output is where the caller asked for it.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mh_internal.h"
#include "mh_k_place.h"

using namespace mh;

struct mh_place_db {
  mh_ctx* ctx = nullptr;
  mh_place_params params{};
  PlaceTables tab{};
  DevBuf desc;          // size * R*S bytes, desc[k][ring * S + sector]
  uint64_t size = 0;
  PinnedBuf h_frames;   // add_frames: page-locked mirror of one pass's upload (points | prefix array | frame table)
};

namespace {

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }
inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
inline bool mem_ok(int32_t mem) { return mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED; }

// The library's own pass size of add_frames: 2 M points are 24 MB of staged coordinates; 4096 frames are at most 64 MB of bins.
constexpr uint64_t kPlacePassPoints = 1ull << 21;
constexpr size_t kPlacePassFrames = 4096;

// the host tables of the specification: fp64, rounded once to fp32.  False: parameters outside the specified ranges.
bool place_make_tables(const mh_place_params* p, PlaceTables& t) {
  if (!p) return false;
  if (p->n_rings < 1 || p->n_rings > MH_PLACE_MAX_RINGS) return false;
  if (p->n_sectors < 8 || p->n_sectors > MH_PLACE_MAX_SECTORS || p->n_sectors % 8) return false;
  if (!(isfinite(p->min_range) && isfinite(p->max_range) && isfinite(p->z_min) && isfinite(p->z_max))) return false;
  if (!(p->min_range >= 0.f && p->min_range < p->max_range && p->z_min < p->z_max)) return false;
  memset(&t, 0, sizeof(t));
  t.R = p->n_rings;
  t.S = p->n_sectors;
  const double r0 = (double)p->min_range, dr = (double)p->max_range - (double)p->min_range;
  for (uint32_t k = 0; k <= t.R; k++) {
    const double e = r0 + (double)k * dr / (double)t.R;
    t.ring_edge2[k] = (float)(e * e);
  }
  for (uint32_t j = 1; j < t.S / 8; j++) t.tan_edge[j] = (float)tan(2.0 * 3.14159265358979323846 * (double)j / (double)t.S);
  t.z_min = p->z_min;
  t.z_max = p->z_max;
  t.zscale = (float)(254.0 / ((double)p->z_max - (double)p->z_min));
  return isfinite(t.ring_edge2[t.R]) && isfinite(t.zscale);  // (ranges whose tables do not fit fp32 are outside the rule)
}

// zero the 32-bit bins of nf frames, bin every point of the pass, narrow to bytes at `d_out` (device memory)
mh_status place_run(hipStream_t s, const PlaceTables& tab, const uint32_t* d_start, const PlaceSrc* d_table, size_t nf, uint64_t P,
                    uint32_t* d_bins32, uint8_t* d_out) {
  const size_t nb = nf * (size_t)tab.R * tab.S;
  MH_HIP(hipMemsetAsync(d_bins32, 0, nb * sizeof(uint32_t), s));
  if (P) hipLaunchKernelGGL(k_place_describe, dim3(nblk(P, kPlaceChunk)), dim3(kPlaceBlock), 0, s, d_start, d_table, (uint32_t)nf, (uint32_t)P, tab, d_bins32);
  hipLaunchKernelGGL(k_place_pack, dim3(nblk(nb, 256)), dim3(256), 0, s, (const uint32_t*)d_bins32, nb, d_out);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

// room for n_total descriptors; what is stored moves along when the block grows (the outgrown block stays valid behind it)
mh_status db_reserve(mh_place_db* db, uint64_t n_total) {
  const size_t RS = (size_t)db->tab.R * db->tab.S;
  void* old = db->desc.p;
  MH_TRY(db->desc.reserve(n_total * RS));
  if (old && old != db->desc.p && db->size)
    MH_HIP(hipMemcpyAsync(db->desc.p, old, db->size * RS, hipMemcpyDeviceToDevice, db->ctx->stream));
  return MH_OK;
}

}  // namespace

extern "C" {

mh_status mh_place_describe(const mh_scan* scan, const mh_place_params* params, uint8_t* desc, int32_t mem) {
  MH_REQUIRE(scan && params && desc, "null argument");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  PlaceTables tab;
  MH_REQUIRE(place_make_tables(params, tab), "descriptor parameters outside their ranges");
  MH_REQUIRE(scan->n < 0xFFFFFFF0ull, "scan size does not fit 32 bits");
  mh_ctx* ctx = scan->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t RS = (size_t)tab.R * tab.S;
  const bool to_device = mem == MH_MEM_DEVICE;
  if (scan->n == 0) {  // an all-zero descriptor
    if (!to_device) {
      memset(desc, 0, RS);
    } else {
      MH_HIP(hipMemsetAsync(desc, 0, RS, s));
      MH_HIP(mh::wait_stream(s));
    }
    return MH_OK;
  }
  // upload: prefix array [2] | frame table [1]; scratch: bins [RS] | bytes [RS]
  struct {
    uint32_t start[64];
    PlaceSrc src;
  } up;
  memset(&up, 0, sizeof(up));
  up.start[1] = (uint32_t)scan->n;
  up.src.x = scan->x; up.src.y = scan->y; up.src.z = scan->z;
  MH_TRY(ctx->staging.reserve(sizeof(up)));
  MH_TRY(ctx->compact.reserve(RS * sizeof(uint32_t) + RS));
  MH_TRY(stage_in(ctx, ctx->staging, 0, &up, sizeof(up), MH_MEM_HOST));
  uint32_t* d_bins = ctx->compact.as<uint32_t>();
  uint8_t* d_bytes = to_device ? desc : (uint8_t*)(d_bins + RS);
  MH_TRY(place_run(s, tab, ctx->staging.as<uint32_t>(), (const PlaceSrc*)(ctx->staging.as<char>() + sizeof(up.start)), 1, scan->n,
                   d_bins, d_bytes));
  if (!to_device) MH_HIP(hipMemcpyAsync(desc, d_bytes, RS, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

mh_status mh_place_db_create(mh_ctx* ctx, const mh_place_params* params, mh_place_db** out) {
  MH_REQUIRE(ctx && params && out, "null argument");
  *out = nullptr;
  PlaceTables tab;
  MH_REQUIRE(place_make_tables(params, tab), "descriptor parameters outside their ranges");
  mh_place_db* db = new (std::nothrow) mh_place_db();
  if (!db) return fail(MH_ERR_OUT_OF_MEMORY, "host allocation failed");
  db->ctx = ctx;
  db->params = *params;
  db->tab = tab;
  *out = db;
  return MH_OK;
}

mh_status mh_place_db_destroy(mh_place_db* db) {
  if (!db) return MH_OK;
  (void)set_device(db->ctx);
  (void)mh::wait_stream(db->ctx->stream);
  db->desc.release();
  db->h_frames.release();
  delete db;
  return MH_OK;
}

mh_status mh_place_db_size(const mh_place_db* db, uint64_t* n) {
  MH_REQUIRE(db && n, "null argument");
  *n = db->size;
  return MH_OK;
}

mh_status mh_place_db_add(mh_place_db* db, const uint8_t* desc, size_t n_desc, int32_t mem) {
  MH_REQUIRE(db, "null database");
  MH_REQUIRE(desc || n_desc == 0, "null descriptors");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  if ((uint64_t)n_desc > (uint64_t)MH_PLACE_MAX_DESCRIPTORS || db->size + n_desc > (uint64_t)MH_PLACE_MAX_DESCRIPTORS)
    return fail(MH_ERR_UNSUPPORTED, "mh_place_db_add: %llu + %zu descriptors exceed MH_PLACE_MAX_DESCRIPTORS (%d)",
                (unsigned long long)db->size, n_desc, MH_PLACE_MAX_DESCRIPTORS);
  if (n_desc == 0) return MH_OK;
  mh_ctx* ctx = db->ctx;
  MH_TRY(set_device(ctx));
  const size_t RS = (size_t)db->tab.R * db->tab.S;
  MH_TRY(db_reserve(db, db->size + n_desc));
  MH_HIP(hipMemcpyAsync(db->desc.as<uint8_t>() + db->size * RS, desc, n_desc * RS,
                        mem == MH_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(mh::wait_stream(ctx->stream));  // the caller's array may be reused
  db->size += n_desc;
  return MH_OK;
}

mh_status mh_place_db_add_frames(mh_place_db* db, const mh_map_frame* frames, size_t n_frames, int32_t mem) {
  MH_REQUIRE(db, "null database");
  MH_REQUIRE(n_frames == 0 || frames, "null frames");
  MH_REQUIRE(mem_ok(mem), "bad mem space");
  for (size_t f = 0; f < n_frames; f++) {
    MH_REQUIRE(frames[f].n == 0 || (frames[f].x && frames[f].y && frames[f].z), "null point arrays");
    MH_REQUIRE(frames[f].n < 0x7FFFFFF0ull, "too many points");
  }
  if ((uint64_t)n_frames > (uint64_t)MH_PLACE_MAX_DESCRIPTORS || db->size + n_frames > (uint64_t)MH_PLACE_MAX_DESCRIPTORS)
    return fail(MH_ERR_UNSUPPORTED, "mh_place_db_add_frames: %llu + %zu descriptors exceed MH_PLACE_MAX_DESCRIPTORS (%d)",
                (unsigned long long)db->size, n_frames, MH_PLACE_MAX_DESCRIPTORS);
  if (n_frames == 0) return MH_OK;
  mh_ctx* ctx = db->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t RS = (size_t)db->tab.R * db->tab.S;
  const bool staged = mem != MH_MEM_DEVICE;  // host arrays travel through the mirror; device arrays are read in place
  MH_TRY(db_reserve(db, db->size + n_frames));
  size_t f0 = 0;
  while (f0 < n_frames) {
    size_t f1 = f0;
    uint64_t P = 0;  // frames in order while they fit; a frame larger than the budget is a pass of its own
    while (f1 < n_frames && f1 - f0 < kPlacePassFrames && (f1 == f0 || P + frames[f1].n <= kPlacePassPoints)) P += frames[f1++].n;
    const size_t nf = f1 - f0;
    // upload layout: [x | y | z of the pass's points (host arrays only)] prefix array [nf + 1] | frame table [nf]
    const size_t pstride = staged ? up256(P * sizeof(float)) : 0;
    const size_t off_start = 3 * pstride;
    const size_t off_table = off_start + up256((nf + 1) * sizeof(uint32_t));
    const size_t up_bytes = off_table + nf * sizeof(PlaceSrc);
    MH_HIP(mh::wait_stream(s));  // the previous pass has read the mirror
    MH_TRY(db->h_frames.reserve(up_bytes));
    MH_TRY(ctx->staging.reserve(up_bytes));
    MH_TRY(ctx->compact.reserve(nf * RS * sizeof(uint32_t)));
    char* h = db->h_frames.as<char>();
    char* d = ctx->staging.as<char>();
    uint32_t* h_start = (uint32_t*)(h + off_start);
    PlaceSrc* h_tab = (PlaceSrc*)(h + off_table);
    uint64_t at = 0;
    for (size_t k = 0; k < nf; k++) {
      const mh_map_frame& fr = frames[f0 + k];
      h_start[k] = (uint32_t)at;
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
    }
    h_start[nf] = (uint32_t)at;
    MH_HIP(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s));  // the pass's one upload
    MH_TRY(place_run(s, db->tab, (const uint32_t*)(d + off_start), (const PlaceSrc*)(d + off_table), nf, P, ctx->compact.as<uint32_t>(),
                     db->desc.as<uint8_t>() + (db->size + f0) * RS));
    f0 = f1;
  }
  MH_HIP(mh::wait_stream(s));  // the caller's arrays may be reused; the descriptors are stored
  db->size += n_frames;
  return MH_OK;
}

mh_status mh_place_search(const mh_place_db* db, const uint8_t* query, int32_t query_mem, mh_place_match* out, int32_t mem) {
  MH_REQUIRE(db && query && out, "null argument");
  MH_REQUIRE(mem_ok(query_mem) && mem_ok(mem), "bad mem space");
  if (db->size == 0) return MH_OK;
  mh_ctx* ctx = db->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t RS = (size_t)db->tab.R * db->tab.S;
  const size_t obytes = db->size * sizeof(mh_place_match);
  const bool to_device = mem == MH_MEM_DEVICE;
  MH_TRY(ctx->staging.reserve(RS));
  if (!to_device) MH_TRY(ctx->compact.reserve(obytes));
  MH_TRY(stage_in(ctx, ctx->staging, 0, query, RS, query_mem == MH_MEM_DEVICE ? MH_MEM_DEVICE : MH_MEM_HOST));
  mh_place_match* d_out = to_device ? out : ctx->compact.as<mh_place_match>();
  const PlaceSearchGeom g = place_search_geom(db->tab.R, db->tab.S);
  const uint32_t n_rounds = nblk(db->size, g.n_sub);
  hipLaunchKernelGGL(k_place_search, dim3(std::min<uint32_t>(n_rounds, 8192u)), dim3(kPlaceBlock), 0, s, db->desc.as<uint32_t>(),
                     (uint32_t)db->size, ctx->staging.as<uint32_t>(), db->tab.R, db->tab.S, d_out);
  MH_HIP(hipGetLastError());
  if (!to_device) MH_HIP(hipMemcpyAsync(out, d_out, obytes, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
