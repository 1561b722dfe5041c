// mh_k_motion.h -- the kernels of include/molahip_motion.h: de-skew with a piecewise motion table.  The
// rule per point is written down in the header; this file restates nothing but its arithmetic order.
//
// One lane per point.  The table (K segments of 13 doubles: knot | R row-major | w) is staged once per workgroup in LDS; a
// layer in raw order is in time order, so the lanes of a wave mostly agree on the segment and read the same LDS words (a
// broadcast, no bank conflict).  The segment is found by a branch-free binary search over the knots: seven probes for any K.
// TABLE_IN_ARG: the table is the kernel argument `arg` (K <= kMotionArgSegs); otherwise it is read from `tab` in device memory.
#pragma once
#include <type_traits>

#include "../../include/molahip_motion.h"
#include "mh_internal.h"
#include "mh_nn_device.h"

namespace mh {
namespace motion {

constexpr uint32_t kSegDoubles = 13;     // sizeof(mh_motion_segment) / 8
constexpr uint32_t kMotionArgSegs = 32;  // the largest table that travels as a kernel argument (3328 bytes)

struct MotionHead {
  double v[3];
  uint32_t K;
};
struct MotionArg {
  double seg[kMotionArgSegs * kSegDoubles];
};
struct MotionNoArg {  // what the launches that read `tab` pass in its place
  double seg[1];
};
template <bool TABLE_IN_ARG>
using MotionArgOf = typename std::conditional<TABLE_IN_ARG, MotionArg, MotionNoArg>::type;

struct MotionLayer {
  const float *x, *y, *z, *t;
  const uint32_t* src;
  const float* i;  // null: no intensity
  float *ox, *oy, *oz, *ot;
  uint32_t* osrc;
  float* oi;
  uint32_t n;
};

template <bool TABLE_IN_ARG>
__device__ __forceinline__ void stage_table(double* __restrict__ sh, const MotionArgOf<TABLE_IN_ARG>& arg, const double* __restrict__ tab, uint32_t K) {
  for (uint32_t k = threadIdx.x; k < K * kSegDoubles; k += blockDim.x) {
    if constexpr (TABLE_IN_ARG) sh[k] = arg.seg[k];
    else sh[k] = G(tab)[k];
  }
  __syncthreads();
}

// s = clamp(#{k : knot_k <= t} - 1, 0, K - 1): the knots ascend, so the count is the largest c with knot_{c-1} <= t
__device__ __forceinline__ uint32_t segment_of(const double* __restrict__ sh, uint32_t K, double t) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t step = 64; step; step >>= 1) {
    const uint32_t j = c + step;
    const uint32_t jj = j <= K ? j : 1u;  // (an address inside the table for the probes beyond it)
    const bool take = (j <= K) & (sh[(jj - 1) * kSegDoubles] <= t);  // false for a NaN stamp
    c = take ? j : c;
  }
  return c ? c - 1 : 0u;
}

__device__ __forceinline__ void motion_point(const double* __restrict__ sh, const MotionHead& h, float x, float y, float z, float tf,
                                             float& gx, float& gy, float& gz) {
  const double t = (double)tf;
  const double* seg = sh + segment_of(sh, h.K, t) * kSegDoubles;
  const double d = t - seg[0];
  const double xi[6] = {0.0, 0.0, 0.0, seg[10] * d, seg[11] * d, seg[12] * d};
  const Pose e = se3_exp(xi);  // zero translation part: pure Exp_SO3(w_s d)
  const double px = x, py = y, pz = z;
  const double ux = (e.R(0, 0) * px + e.R(0, 1) * py) + e.R(0, 2) * pz;
  const double uy = (e.R(1, 0) * px + e.R(1, 1) * py) + e.R(1, 2) * pz;
  const double uz = (e.R(2, 0) * px + e.R(2, 1) * py) + e.R(2, 2) * pz;
  gx = (float)(((seg[1] * ux + seg[2] * uy) + seg[3] * uz) + h.v[0] * t);
  gy = (float)(((seg[4] * ux + seg[5] * uy) + seg[6] * uz) + h.v[1] * t);
  gz = (float)(((seg[7] * ux + seg[8] * uy) + seg[9] * uz) + h.v[2] * t);
}

__device__ __forceinline__ void motion_lane(const double* __restrict__ sh, const MotionHead& h, const MotionLayer& l, uint32_t i,
                                            float& gx, float& gy, float& gz) {
  const float tf = G(l.t)[i];
  G(l.ot)[i] = tf;
  if (l.src) G(l.osrc)[i] = G(l.src)[i];
  if (l.i) G(l.oi)[i] = G(l.i)[i];
  motion_point(sh, h, G(l.x)[i], G(l.y)[i], G(l.z)[i], tf, gx, gy, gz);
  G(l.ox)[i] = gx;
  G(l.oy)[i] = gy;
  G(l.oz)[i] = gz;
}

template <bool TABLE_IN_ARG>
__global__ __launch_bounds__(256) void k_motion_deskew(MotionLayer l, MotionHead h, MotionArgOf<TABLE_IN_ARG> arg, const double* __restrict__ tab) {
  __shared__ double sh[MH_MOTION_MAX_SEGMENTS * kSegDoubles];
  stage_table<TABLE_IN_ARG>(sh, arg, tab, h.K);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= l.n) return;
  float gx, gy, gz;
  motion_lane(sh, h, l, i, gx, gy, gz);
}

__device__ __forceinline__ uint32_t f2ord(float f) {  // (the order-preserving word of mh_scan_bbox)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Both layers of a scan in one launch, the shape of k_pp_deskew_pair: workgroup 0 walks the small layer and reduces the box of
// what it wrote -- min[3] | max[3] as ordered words | finite count -- straight into page-locked host memory; the others take
// 1024 points of the large layer each.
template <bool TABLE_IN_ARG>
__global__ __launch_bounds__(1024) void k_motion_deskew_pair(MotionLayer big, MotionLayer small, MotionHead h, MotionArgOf<TABLE_IN_ARG> arg,
                                                             const double* __restrict__ tab, uint32_t* __restrict__ host_out) {
  __shared__ double sh[MH_MOTION_MAX_SEGMENTS * kSegDoubles];
  __shared__ uint32_t red[16][7];
  stage_table<TABLE_IN_ARG>(sh, arg, tab, h.K);
  if (blockIdx.x > 0) {
    const uint32_t i = (blockIdx.x - 1) * 1024u + threadIdx.x;
    if (i >= big.n) return;
    float gx, gy, gz;
    motion_lane(sh, h, big, i, gx, gy, gz);
    return;
  }
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, cnt = 0;
  for (uint32_t i = threadIdx.x; i < small.n; i += 1024u) {
    float p[3];
    motion_lane(sh, h, small, i, p[0], p[1], p[2]);
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const uint32_t o = f2ord(p[a]);
        mn[a] = min(mn[a], o);
        mx[a] = max(mx[a], o);
      }
      cnt++;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      mn[a] = min(mn[a], (uint32_t)__shfl_xor((int)mn[a], off));
      mx[a] = max(mx[a], (uint32_t)__shfl_xor((int)mx[a], off));
    }
    cnt += (uint32_t)__shfl_xor((int)cnt, off);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { red[w][a] = mn[a]; red[w][3 + a] = mx[a]; }
    red[w][6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int a = threadIdx.x;
    uint32_t v = red[0][a];
    for (int q = 1; q < 16; q++) v = a < 3 ? min(v, red[q][a]) : (a < 6 ? max(v, red[q][a]) : v + red[q][a]);
    host_out[a] = v;
  }
}

}  // namespace motion
}  // namespace mh
