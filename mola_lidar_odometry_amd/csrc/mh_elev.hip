// mh_elev.hip -- the entry points of include/molahip_elevation.h: the index bounds of a group of posed
// key-frames, the elevation map's two point passes, the relief stencil and the download.  The reading is written down in the
// header; the kernels are mh_k_elev.h's; refusals, passes and staging are the ones mh_map_insert_frames uses (mh_frames_pass.h).
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <new>

#include "../../include/molahip_elevation.h"
#include "mh_frames_pass.h"
#include "mh_k_elev.h"

using namespace mh;
using namespace mh::elev;

namespace {

inline uint32_t nblk(size_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// what a point pass needs besides the planes: the mirror and the device block of one pass's upload, the counters
struct PassScratch {
  PinnedBuf h_up, h_ctr;  // h_ctr: Counters[2] = {what a pass starts from, what it left}
  DevBuf up, ctr;
  void release() {
    h_up.release();
    h_ctr.release();
    up.release();
    ctr.release();
  }
};

struct PassTotals {
  uint64_t points = 0, left_out = 0, outside = 0, n_in = 0;
  int lo[2] = {INT_MAX, INT_MAX}, hi[2] = {INT_MIN, INT_MIN};
};

struct Planes {
  int* ground = nullptr;
  uint32_t* count = nullptr;
  uint32_t* obstacle = nullptr;
  int* top = nullptr;
};

// The frames in passes through k_elev_points<MODE>.  `t` takes a pass in once it is complete; a failure leaves it at the totals of
// the completed passes, with nothing in flight.
template <int MODE>
mh_status run_passes(mh_ctx* ctx, PassScratch& sc, const mh_map_frame* frames, size_t n_frames, int32_t mem, uint64_t max_points_per_pass,
                     float inv, float invq, float max_range, const Window& w, int clearance_q, int step_q, const Planes& pl,
                     PassTotals& t) {
  hipStream_t s = ctx->stream;
  const uint64_t budget = std::min<uint64_t>(max_points_per_pass ? max_points_per_pass : kFramesPassPoints, 0x7FFFFFEFull);
  const bool staged = mem != MH_MEM_DEVICE;
  const float max_range2 = max_range > 0.f ? max_range * max_range : -1.f;
  auto pass = [&](size_t f0, size_t nf, uint64_t P) -> mh_status {
    const FramesUpload up = frames_upload_layout(nf, P, staged, sizeof(FrameSrc));
    MH_TRY(sc.h_up.reserve(up.bytes));
    MH_TRY(sc.up.reserve(up.bytes));
    MH_TRY(sc.h_ctr.reserve(2 * sizeof(Counters)));
    MH_TRY(sc.ctr.reserve(sizeof(Counters)));
    char* h = sc.h_up.as<char>();
    char* d = sc.up.as<char>();
    frames_fill_upload<FrameSrc>(up, frames + f0, nf, staged, h, d);
    Counters* hc = sc.h_ctr.as<Counters>();
    hc[0] = Counters{};
    hc[0].lo[0] = hc[0].lo[1] = INT_MAX;
    hc[0].hi[0] = hc[0].hi[1] = INT_MIN;
    MH_HIP(hipMemcpyAsync(d, h, up.bytes, hipMemcpyHostToDevice, s));  // the pass's one upload
    MH_HIP(hipMemcpyAsync(sc.ctr.p, &hc[0], sizeof(Counters), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_elev_points<MODE>, dim3(nblk(P, 256)), dim3(256), 0, s, (const uint32_t*)(d + up.off_start),
                       (const FrameSrc*)(d + up.off_table), (uint32_t)nf, (uint32_t)P, inv, invq, max_range2, w, clearance_q, step_q,
                       pl.ground, pl.count, pl.obstacle, pl.top, sc.ctr.as<Counters>());
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&hc[1], sc.ctr.p, sizeof(Counters), hipMemcpyDeviceToHost, s));
    MH_HIP(mh::wait_stream(s));  // (the mirror and the caller's arrays are free again behind this)
    uint64_t left_out = 0;
    for (uint32_t k = 0; k < kCounterSlots; k++) {
      left_out += hc[1].slot[k].left_out;
      t.outside += hc[1].slot[k].outside;
    }
    t.points += P;
    t.left_out += left_out;
    t.n_in += P - left_out;  // (the bounds pass: every point that is not left out is in)
    for (int a = 0; a < 2; a++) {
      t.lo[a] = std::min(t.lo[a], hc[1].lo[a]);
      t.hi[a] = std::max(t.hi[a], hc[1].hi[a]);
    }
    return MH_OK;
  };
  size_t f0 = 0;
  while (f0 < n_frames) {
    uint64_t P = 0;
    const size_t f1 = frames_next_pass(frames, n_frames, f0, budget, &P);
    if (P == 0) break;  // (only empty frames were left)
    const mh_status st = pass(f0, f1 - f0, P);
    if (st != MH_OK) {
      (void)mh::wait_stream(s);  // (nothing may still read the mirror or the caller's arrays)
      return st;
    }
    f0 = f1;
  }
  return MH_OK;
}

}  // namespace

struct mh_elev {
  mh_ctx* ctx = nullptr;
  mh_elev_params params{};
  float inv = 1.f, invq = 1.f;
  size_t n_cells = 0;
  DevBuf planes;  // ground | count | obstacle_count | top, n_cells entries each
  DevBuf relief;
  PassScratch sc;
  mh_elev_info info{};
  Planes view() const {
    Planes p;
    p.ground = planes.as<int>();
    p.count = planes.as<uint32_t>() + n_cells;
    p.obstacle = planes.as<uint32_t>() + 2 * n_cells;
    p.top = planes.as<int>() + 3 * n_cells;
    return p;
  }
  Window window() const { return Window{params.x0, params.y0, params.nx, params.ny}; }
};

namespace {

mh_status elev_fill(mh_elev* e) {
  const Planes p = e->view();
  hipLaunchKernelGGL(k_elev_fill, dim3(nblk(e->n_cells, 256)), dim3(256), 0, e->ctx->stream, p.ground, p.count, p.obstacle, p.top,
                     e->n_cells);
  MH_HIP(hipGetLastError());
  MH_HIP(mh::wait_stream(e->ctx->stream));
  e->info = mh_elev_info{};
  return MH_OK;
}

}  // namespace

extern "C" {

uint32_t mh_elev_api_version(void) { return MH_ELEV_API_VERSION; }

mh_status mh_elev_bounds_frames(mh_ctx* ctx, const mh_map_frame* frames, size_t n_frames, int32_t mem, float resolution,
                                float max_range, uint64_t max_points_per_pass, int32_t lo[2], int32_t hi[2], uint64_t* n_in) {
  MH_REQUIRE(ctx && lo && hi && n_in, "null argument");
  MH_REQUIRE(isfinite(resolution) && resolution > 0.f, "resolution must be finite and > 0");
  MH_REQUIRE(isfinite(max_range) && max_range >= 0.f, "max_range must be finite and >= 0");
  uint64_t sum = 0;
  MH_TRY(frames_check(__func__, frames, n_frames, mem, &sum));
  *n_in = 0;
  if (sum == 0) return MH_OK;
  MH_TRY(set_device(ctx));
  PassScratch sc;
  PassTotals t;
  const mh_status st = run_passes<kBounds>(ctx, sc, frames, n_frames, mem, max_points_per_pass, 1.0f / resolution, 1.0f, max_range,
                                           Window{0, 0, 0u, 0u}, 0, 0, Planes{}, t);
  sc.release();
  MH_TRY(st);
  *n_in = t.n_in;
  if (t.n_in) {
    for (int a = 0; a < 2; a++) {
      lo[a] = t.lo[a];
      hi[a] = t.hi[a];
    }
  }
  return MH_OK;
}

mh_status mh_elev_create(mh_ctx* ctx, const mh_elev_params* p, mh_elev** out) {
  MH_REQUIRE(ctx && p && out, "null argument");
  MH_REQUIRE(isfinite(p->resolution) && p->resolution > 0.f, "resolution must be finite and > 0");
  MH_REQUIRE(isfinite(p->z_quantum) && p->z_quantum > 0.f, "z_quantum must be finite and > 0");
  MH_REQUIRE(isfinite(p->max_range) && p->max_range >= 0.f, "max_range must be finite and >= 0");
  MH_REQUIRE(p->nx > 0 && p->ny > 0, "nx and ny must be > 0");
  MH_REQUIRE((uint64_t)p->nx * (uint64_t)p->ny <= (1ull << 26), "nx * ny must not exceed 2^26");
  MH_REQUIRE(p->clearance_q >= 0 && p->step_q >= 0, "clearance_q and step_q must be >= 0");
  MH_TRY(set_device(ctx));
  mh_elev* e = new (std::nothrow) mh_elev();
  if (!e) return fail(MH_ERR_OUT_OF_MEMORY, "mh_elev_create: out of host memory");
  e->ctx = ctx;
  e->params = *p;
  e->inv = 1.0f / p->resolution;
  e->invq = 1.0f / p->z_quantum;
  e->n_cells = (size_t)p->nx * p->ny;
  mh_status st = e->planes.reserve(4 * e->n_cells * sizeof(int));
  if (st == MH_OK) st = elev_fill(e);
  if (st != MH_OK) {
    (void)mh_elev_destroy(e);
    return st;
  }
  *out = e;
  return MH_OK;
}

mh_status mh_elev_destroy(mh_elev* e) {
  if (!e) return MH_OK;
  (void)set_device(e->ctx);
  (void)mh::wait_stream(e->ctx->stream);
  e->planes.release();
  e->relief.release();
  e->sc.release();
  delete e;
  return MH_OK;
}

mh_status mh_elev_clear(mh_elev* e) {
  MH_REQUIRE(e, "null map");
  MH_TRY(set_device(e->ctx));
  return elev_fill(e);
}

mh_status mh_elev_get_info(const mh_elev* e, mh_elev_info* info) {
  MH_REQUIRE(e && info, "null argument");
  *info = e->info;
  return MH_OK;
}

mh_status mh_elev_add_frames(mh_elev* e, const mh_map_frame* frames, size_t n_frames, int32_t mem, uint64_t max_points_per_pass) {
  MH_REQUIRE(e, "null map");
  uint64_t sum = 0;
  MH_TRY(frames_check(__func__, frames, n_frames, mem, &sum));
  MH_REQUIRE(!e->info.ground_frozen, "the ground is frozen by mh_elev_mark_frames: mh_elev_clear starts over");
  MH_REQUIRE(e->info.n_counted + sum <= 0xFFFFFFF0ull, "too many points");
  if (sum == 0) return MH_OK;
  MH_TRY(set_device(e->ctx));
  PassTotals t;
  const mh_status st = run_passes<kAdd>(e->ctx, e->sc, frames, n_frames, mem, max_points_per_pass, e->inv, e->invq, e->params.max_range,
                                        e->window(), e->params.clearance_q, e->params.step_q, e->view(), t);
  e->info.n_offered += t.points;
  e->info.n_left_out += t.left_out;
  e->info.n_outside_window += t.outside;
  e->info.n_counted += t.points - t.left_out - t.outside;
  return st;
}

mh_status mh_elev_mark_frames(mh_elev* e, const mh_map_frame* frames, size_t n_frames, int32_t mem, uint64_t max_points_per_pass) {
  MH_REQUIRE(e, "null map");
  uint64_t sum = 0;
  MH_TRY(frames_check(__func__, frames, n_frames, mem, &sum));
  MH_REQUIRE(e->info.n_mark_offered - e->info.n_mark_left_out - e->info.n_mark_outside_window + sum <= 0xFFFFFFF0ull, "too many points");
  if (sum == 0) return MH_OK;
  MH_TRY(set_device(e->ctx));
  e->info.ground_frozen = 1u;
  PassTotals t;
  const mh_status st = run_passes<kMark>(e->ctx, e->sc, frames, n_frames, mem, max_points_per_pass, e->inv, e->invq, e->params.max_range,
                                         e->window(), e->params.clearance_q, e->params.step_q, e->view(), t);
  e->info.n_mark_offered += t.points;
  e->info.n_mark_left_out += t.left_out;
  e->info.n_mark_outside_window += t.outside;
  return st;
}

mh_status mh_elev_relief(const mh_elev* e, uint32_t radius, uint32_t min_points, int32_t* relief_host) {
  MH_REQUIRE(e && relief_host, "null argument");
  MH_REQUIRE(radius <= MH_ELEV_MAX_RELIEF_RADIUS, "radius must not exceed 4");
  MH_REQUIRE(min_points >= 1, "min_points must be >= 1");
  mh_elev* w = const_cast<mh_elev*>(e);  // (scratch is the handle's)
  MH_TRY(set_device(e->ctx));
  hipStream_t s = e->ctx->stream;
  MH_TRY(w->relief.reserve(e->n_cells * sizeof(int)));
  const Planes p = e->view();
  hipLaunchKernelGGL(k_elev_relief, dim3(nblk(e->params.nx, kTileX) * nblk(e->params.ny, kTileY)), dim3(256), 0, s, p.ground, p.count,
                     e->params.nx, e->params.ny, (int)radius, min_points, w->relief.as<int>());
  MH_HIP(hipGetLastError());
  MH_HIP(hipMemcpyAsync(relief_host, w->relief.p, e->n_cells * sizeof(int), hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

mh_status mh_elev_download(const mh_elev* e, int32_t* ground, uint32_t* count, uint32_t* obstacle_count, int32_t* top) {
  MH_REQUIRE(e, "null map");
  MH_TRY(set_device(e->ctx));
  hipStream_t s = e->ctx->stream;
  const Planes p = e->view();
  const size_t b = e->n_cells * sizeof(int);
  if (ground) MH_HIP(hipMemcpyAsync(ground, p.ground, b, hipMemcpyDeviceToHost, s));
  if (count) MH_HIP(hipMemcpyAsync(count, p.count, b, hipMemcpyDeviceToHost, s));
  if (obstacle_count) MH_HIP(hipMemcpyAsync(obstacle_count, p.obstacle, b, hipMemcpyDeviceToHost, s));
  if (top) MH_HIP(hipMemcpyAsync(top, p.top, b, hipMemcpyDeviceToHost, s));
  MH_HIP(mh::wait_stream(s));
  return MH_OK;
}

}  // extern "C"
