// mh_motion.hip -- the entry points of include/molahip_motion.h: de-skew with a piecewise motion table.
// The rule, the fall-backs and how the table travels are written down in the header; the kernels are mh_k_motion.h's.
#include <math.h>
#include <string.h>

#include "../../include/molahip_motion.h"
#include "mh_k_motion.h"

using namespace mh;
using namespace mh::motion;

static_assert(sizeof(mh_motion_segment) == kSegDoubles * sizeof(double), "a segment is 13 doubles");
static_assert(sizeof(mh_motion_table) == 40, "mh_motion_table is 40 bytes");

namespace {

// every refusal that concerns the table alone
mh_status check_table(const char* who, const mh_motion_table* m) {
  if (m->n_segments < 1 || m->n_segments > MH_MOTION_MAX_SEGMENTS)
    return mh::fail(MH_ERR_INVALID_ARGUMENT, "%s: n_segments must be in 1..MH_MOTION_MAX_SEGMENTS", who);
  if (!m->segments) return mh::fail(MH_ERR_INVALID_ARGUMENT, "%s: null segments", who);
  for (int a = 0; a < 3; a++)
    if (!isfinite(m->v[a])) return mh::fail(MH_ERR_INVALID_ARGUMENT, "%s: non-finite v", who);
  for (uint32_t k = 0; k < m->n_segments; k++) {
    const mh_motion_segment& s = m->segments[k];
    bool ok = isfinite(s.knot);
    for (int a = 0; a < 9; a++) ok = ok && isfinite(s.R[a]);
    for (int a = 0; a < 3; a++) ok = ok && isfinite(s.w[a]);
    if (!ok) return mh::fail(MH_ERR_INVALID_ARGUMENT, "%s: non-finite knot, R or w in segment %u", who, k);
    if (k && !(m->segments[k - 1].knot < s.knot))
      return mh::fail(MH_ERR_INVALID_ARGUMENT, "%s: knots must ascend strictly (segment %u)", who, k);
  }
  return MH_OK;
}

MotionHead head_of(const mh_motion_table* m) {
  MotionHead h;
  for (int a = 0; a < 3; a++) h.v[a] = m->v[a];
  h.K = m->n_segments;
  return h;
}

MotionLayer layer_of(const mh_scan* in, mh_scan* out) {
  MotionLayer l;
  l.x = in->x; l.y = in->y; l.z = in->z; l.t = in->t; l.src = in->src; l.i = in->i;
  l.ox = (float*)out->x; l.oy = (float*)out->y; l.oz = (float*)out->z; l.ot = (float*)out->t; l.osrc = (uint32_t*)out->src;
  l.oi = (float*)out->i;
  l.n = (uint32_t)in->n;
  return l;
}

// A table above kMotionArgSegs segments: a stream-ordered copy from the caller's pageable block (staged before the copy call
// returns) into the context's block; the launch that reads it follows on the same stream, the next call's copy behind that.
mh_status table_to_device(mh_ctx* ctx, hipStream_t s, const mh_motion_table* m, const double** d_tab) {
  const size_t bytes = (size_t)m->n_segments * sizeof(mh_motion_segment);
  MH_TRY(ctx->build_e.reserve(bytes));
  MH_HIP(hipMemcpyAsync(ctx->build_e.p, m->segments, bytes, hipMemcpyHostToDevice, s));
  *d_tab = ctx->build_e.as<double>();
  return MH_OK;
}

void bbox_from_words(const uint32_t h[7], float bb_min[3], float bb_max[3], uint64_t* n_finite) {  // (as mh_scan_bbox reads them)
  auto ord = [](uint32_t u) { u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u; float f; memcpy(&f, &u, 4); return f; };
  for (int a = 0; a < 3; a++) {
    bb_min[a] = h[6] ? ord(h[a]) : 0.f;
    bb_max[a] = h[6] ? ord(h[3 + a]) : 0.f;
  }
  if (n_finite) *n_finite = h[6];
}

}  // namespace

extern "C" {

uint32_t mh_motion_api_version(void) { return MH_MOTION_API_VERSION; }

mh_status mh_scan_deskew_motion(const mh_scan* in, const mh_motion_table* motion, mh_scan* out) {
  MH_REQUIRE(in && out, "null argument");
  MH_REQUIRE(in != out, "`out` must differ from `in`");
  MH_REQUIRE(in->ctx->device == out->ctx->device, "scans live on different devices");
  if (motion) MH_TRY(check_table(__func__, motion));
  if (!motion || !in->t) return mh_scan_deskew(in, nullptr, out);  // the copies of mh_scan_deskew, channel by channel
  mh_ctx* ctx = out->ctx;
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  const size_t n = in->n;
  MH_TRY(scan_alloc(out, n, true, in->src != nullptr, in->i != nullptr));
  if (!n) return MH_OK;
  const MotionHead h = head_of(motion);
  const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
  if (h.K <= kMotionArgSegs) {
    MotionArg arg;
    memset(&arg, 0, sizeof(arg));
    memcpy(arg.seg, motion->segments, h.K * sizeof(mh_motion_segment));
    hipLaunchKernelGGL(k_motion_deskew<true>, grid, block, 0, s, layer_of(in, out), h, arg, (const double*)nullptr);
  } else {
    const double* d_tab = nullptr;
    MH_TRY(table_to_device(ctx, s, motion, &d_tab));
    hipLaunchKernelGGL(k_motion_deskew<false>, grid, block, 0, s, layer_of(in, out), h, MotionNoArg{{0.0}}, d_tab);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

mh_status mh_scan_deskew_motion_pair(const mh_scan* in_a, const mh_scan* in_b, const mh_motion_table* motion, mh_scan* out_a,
                                     mh_scan* out_b, float bb_min[3], float bb_max[3], uint64_t* n_finite) {
  MH_REQUIRE(in_a && in_b && out_a && out_b && bb_min && bb_max, "null argument");
  MH_REQUIRE(in_a != out_a && in_b != out_b && out_a != out_b && in_a != out_b && in_b != out_a, "the four scans must be distinct");
  MH_REQUIRE(out_a->ctx == out_b->ctx, "the outputs belong to different contexts");
  mh_ctx* ctx = out_a->ctx;
  MH_REQUIRE(in_a->ctx->device == ctx->device && in_b->ctx->device == ctx->device, "scans live on different devices");
  if (motion) MH_TRY(check_table(__func__, motion));
  const bool fused = motion && in_a->t && in_b->t && in_a->n && in_b->n && in_b->n <= 65536 && in_a->n < 0x7FFFFF00ull;
  if (!fused) {  // copies (no table / no time stamps), empty or huge layers: the separate calls
    MH_TRY(mh_scan_deskew_motion(in_a, motion, out_a));
    MH_TRY(mh_scan_deskew_motion(in_b, motion, out_b));
    return mh_scan_bbox(out_b, bb_min, bb_max, n_finite);
  }
  MH_TRY(set_device(ctx));
  hipStream_t s = ctx->stream;
  MH_TRY(scan_alloc(out_a, in_a->n, true, in_a->src != nullptr, in_a->i != nullptr));
  MH_TRY(scan_alloc(out_b, in_b->n, true, in_b->src != nullptr, in_b->i != nullptr));
  if (!ctx->h_small) MH_HIP(hipHostMalloc((void**)&ctx->h_small, 64 * sizeof(uint32_t), hipHostMallocDefault));
  const MotionHead h = head_of(motion);
  const dim3 grid(1 + (uint32_t)((in_a->n + 1023) / 1024)), block(1024);
  if (h.K <= kMotionArgSegs) {
    MotionArg arg;
    memset(&arg, 0, sizeof(arg));
    memcpy(arg.seg, motion->segments, h.K * sizeof(mh_motion_segment));
    hipLaunchKernelGGL(k_motion_deskew_pair<true>, grid, block, 0, s, layer_of(in_a, out_a), layer_of(in_b, out_b), h, arg,
                       (const double*)nullptr, ctx->h_small);
  } else {
    const double* d_tab = nullptr;
    MH_TRY(table_to_device(ctx, s, motion, &d_tab));
    hipLaunchKernelGGL(k_motion_deskew_pair<false>, grid, block, 0, s, layer_of(in_a, out_a), layer_of(in_b, out_b), h,
                       MotionNoArg{{0.0}}, d_tab, ctx->h_small);
  }
  MH_HIP(hipGetLastError());
  MH_HIP(mh::wait_stream(s));
  uint32_t w[7];
  for (int a = 0; a < 7; a++) w[a] = ctx->h_small[a];
  bbox_from_words(w, bb_min, bb_max, n_finite);
  return MH_OK;
}

}  // extern "C"
