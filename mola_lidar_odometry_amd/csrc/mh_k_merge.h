// mh_k_merge.h -- the clouds of several sensors of one rig merged into one vehicle-frame layer (included by mh_preprocess.hip;
// semantics in include/molahip.h at mh_scan_merge_sensors).  What mola::LidarOdometry::onLidarImpl does per observation of a
// synchronised group on the CPU (LidarOdometry.cpp:704-721: the generator applies the sensor pose, FilterAdjustTimestamps runs
// with that sensor's SENSOR_TIME_OFFSET, metric_map_t::merge_with appends) is two launches here, whatever the number of sources:
//   k_merge_tminmax: min / max of the stamps of every source that adjusts them, grid.y = source (the shape of k_pp_tminmax_b)
//   k_merge_fill:    one lane per OUTPUT point; it finds its source in a table of nine start offsets, reads that source's
//                    pose / method / offset from the same table and writes the transformed point.
// The table (MergeTable) is built on the host and travels in ONE copy that also initialises the min / max words.  It lives in
// device memory and not in the kernel arguments: a lane indexes it with ITS source, and a by-value argument indexed per lane
// is copied to scratch first.
#pragma once

namespace {

__device__ __forceinline__ uint32_t merge_ord(float f) {  // (f2ord of k_pp_tminmax_b)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float merge_unord(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(u);
}

struct MergeSrc {
  const float *x, *y, *z, *t, *i;  // the source's channels (t / i null: the output carries none either)
  double P[12];                    // sensor on the vehicle, row-major 3x4
  uint32_t n;
  int32_t method;                  // MH_TS_*, MH_TS_NONE for a source without stamps
  float offset;
  uint32_t pad_;
};

struct MergeTable {
  uint32_t start[MH_MAX_MERGE_SOURCES + 1];  // first output index of every source; entries past the last source = the total
  uint32_t pad_[3];
  uint32_t mm[MH_MAX_MERGE_SOURCES][2];      // ordered-uint min / max of the stamps, {0xFFFFFFFF, 0} from the host
  MergeSrc s[MH_MAX_MERGE_SOURCES];
};

// grid-stride over a small fixed grid.x, one pair of atomics per workgroup; sources that keep their stamps leave at once
__global__ __launch_bounds__(256) void k_merge_tminmax(MergeTable* __restrict__ tab) {
  const MergeSrc& s = tab->s[blockIdx.y];
  if (s.method == MH_TS_NONE || !s.n) return;  // (uniform)
  __shared__ uint32_t smn[4], smx[4];
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
  const float MH_AS_GLOBAL* gt = mh::G(s.t);
  const uint32_t n = s.n;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t o = merge_ord(gt[i]);
    mn = min(mn, o);
    mx = max(mx, o);
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, off));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
  }
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = min(min(smn[0], smn[1]), min(smn[2], smn[3]));
    mx = max(max(smx[0], smx[1]), max(smx[2], smx[3]));
    if (mn != 0xFFFFFFFFu) {
      atomicMin(&tab->mm[blockIdx.y][0], mn);
      atomicMax(&tab->mm[blockIdx.y][1], mx);
    }
  }
}

// One lane per output point.  The start offsets are read with uniform addresses (scalar loads); the lane's source is the
// number of offsets at or below its index -- empty sources repeat an offset and are stepped over, the unused entries hold
// the total, so the count stays below the number of sources.  Lanes of one wave may belong to different sources: everything
// after the search is per lane.  Loads and stores are coalesced SoA inside a source.
__global__ __launch_bounds__(256) void k_merge_fill(const MergeTable* __restrict__ tab, uint32_t total, float* __restrict__ ox,
                                                    float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ ot,
                                                    float* __restrict__ oi) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  uint32_t k = 0, base = 0;
#pragma unroll
  for (int c = 1; c < MH_MAX_MERGE_SOURCES; c++) {
    const uint32_t st = tab->start[c];
    if (q >= st) {
      k = (uint32_t)c;
      base = st;
    }
  }
  const MergeSrc& s = tab->s[k];
  const uint32_t j = q - base;
  double P[12];
#pragma unroll
  for (int c = 0; c < 12; c++) P[c] = s.P[c];
  float gx, gy, gz;
  mh::transform_point(P, mh::G(s.x)[j], mh::G(s.y)[j], mh::G(s.z)[j], gx, gy, gz);
  ox[q] = gx;
  oy[q] = gy;
  oz[q] = gz;
  if (ot) {
    float tv = mh::G(s.t)[j];
    const int32_t method = s.method;
    if (method != MH_TS_NONE) {  // FilterAdjustTimestamps over THIS source's stamps (k_pp_compact_b's arithmetic)
      const float tmin = merge_unord(tab->mm[k][0]), tmax = merge_unord(tab->mm[k][1]);
      const float dt = method == MH_TS_MIDDLE_IS_ZERO ? 0.5f * (tmin + tmax) : tmin;
      tv = (tv - dt) + s.offset;
    }
    ot[q] = tv;
  }
  if (oi) oi[q] = mh::G(s.i)[j];
}

}  // namespace
