// mh_k_rimg.h -- GeneratorEdgesFromRangeImage [U] on the device (included by mh_preprocess.hip; semantics in
// include/molahip.h at mh_scan_edges_from_range_image): a 1-D stencil of radius W along the rows of a 16-bit range image
// sorts every scored pixel into edges or planes, then the ordered compaction of the curvature filter (mh_k_curv.h): the
// same packed class words (edges in field 0, planes in field 1), the same single scan, and a scatter of its own that
// recomputes each kept pixel's point from (r, c, R) -- no xyz image is ever written.
#pragma once

namespace {

constexpr uint32_t kRimgSeg = 256;      // columns of a row one workgroup owns
constexpr uint32_t kRimgMaxW = 64;      // row_window_length (the halo on either side)
enum : uint32_t { kRimgEdge = 1, kRimgPlane = 2 };  // (field of the packed word = class - 1)

struct RimgCam {
  float fx, fy, cx, cy, units;
  uint32_t is_depth;
  double P[12];
};

// One workgroup per (row, segment of 256 columns): segment + 2W samples staged in LDS once (zero outside the row: such
// windows are unscored anyway), then every lane sums its window from LDS.  2W+1 LDS reads per lane, neighbouring lanes
// sharing or neighbouring a bank: 13 reads at rgbd.yaml's W = 6.
// Grid: rows * nseg workgroups in one dimension (a tall image has more rows than a grid's y extent).
__global__ __launch_bounds__(kRimgSeg) void k_rimg_classify(const uint16_t* __restrict__ range, uint32_t rows, uint32_t cols,
                                                            uint32_t nseg, uint32_t W, float thr, uint32_t n, uint32_t cap,
                                                            unsigned long long* __restrict__ word) {
  __shared__ uint16_t sm[kRimgSeg + 2 * kRimgMaxW];
  const uint32_t r = blockIdx.x / nseg, seg = blockIdx.x - r * nseg, c0 = seg * kRimgSeg, tid = threadIdx.x;
  const uint16_t* row = range + (size_t)r * cols;
  for (uint32_t j = tid; j < kRimgSeg + 2 * W; j += kRimgSeg) {
    const int64_t c = (int64_t)c0 + j - W;
    sm[j] = (c >= 0 && c < (int64_t)cols) ? row[c] : (uint16_t)0;
  }
  // the padding up to `cap`, which the scan runs over (fewer than 256 words: one workgroup's lanes)
  if (seg == 0 && r + 1 == rows && n + tid < cap) word[n + tid] = 0ull;
  __syncthreads();
  const uint32_t c = c0 + tid;
  if (c >= cols) return;
  uint32_t cls = 0;
  if (c >= W && c + W < cols) {
    uint32_t sum = 0;
    bool all = true;
    for (uint32_t k = 0; k <= 2 * W; k++) {
      const uint32_t v = sm[tid + k];
      sum += v;
      all = all && v != 0u;
    }
    if (all) {
      const int32_t S = (int32_t)sum - (int32_t)((2 * W + 1) * (uint32_t)sm[tid + W]);
      cls = (float)(S < 0 ? -S : S) > thr ? kRimgEdge : kRimgPlane;
    }
  }
  word[(size_t)r * cols + c] = cls ? 1ull << (kCurvFieldBits * (cls - 1u)) : 0ull;
}

struct RimgOut {
  float *x, *y, *z;
  uint32_t* src;  // null: this output was not asked for
};

// every scored pixel to its place in its layer, its point computed here; the first lane also writes the two counts (the
// scan's total) to page-locked host memory
__global__ __launch_bounds__(256) void k_rimg_scatter(const uint16_t* __restrict__ range, uint32_t cols, uint32_t n, uint32_t cap,
                                                      RimgCam cam, const unsigned long long* __restrict__ word,
                                                      const unsigned long long* __restrict__ pos, RimgOut o0, RimgOut o1,
                                                      uint32_t* __restrict__ host_counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr unsigned long long kMask = (1ull << kCurvFieldBits) - 1ull;
  if (i == 0) {
    const unsigned long long total = pos[cap - 1] + word[cap - 1];
    host_counts[0] = (uint32_t)(total & kMask);
    host_counts[1] = (uint32_t)((total >> kCurvFieldBits) & kMask);
  }
  if (i >= n) return;
  const unsigned long long w = word[i];
  if (!w) return;
  const uint32_t f = w == 1ull ? 0u : 1u;
  uint32_t* osrc = f == 0u ? o0.src : o1.src;
  if (!osrc) return;
  const uint32_t r = i / cols, c = i - r * cols;
  // (-ffp-contract=off and HIP's default correctly rounded divide and square root: the restatement's own ops)
  const float d = (float)range[i] * cam.units;
  const float kx = (cam.cx - (float)c) / cam.fx;
  const float ky = (cam.cy - (float)r) / cam.fy;
  float xs;
  if (cam.is_depth) {
    xs = d;
  } else {
    xs = (float)((double)d / sqrt((1.0 + (double)kx * (double)kx) + (double)ky * (double)ky));
  }
  const float ys = xs * kx, zs = xs * ky;
  const double X = xs, Y = ys, Z = zs;
  const uint32_t k = (uint32_t)((pos[i] >> (kCurvFieldBits * f)) & kMask);
  (f == 0u ? o0.x : o1.x)[k] = (float)(((cam.P[0] * X + cam.P[1] * Y) + cam.P[2] * Z) + cam.P[3]);
  (f == 0u ? o0.y : o1.y)[k] = (float)(((cam.P[4] * X + cam.P[5] * Y) + cam.P[6] * Z) + cam.P[7]);
  (f == 0u ? o0.z : o1.z)[k] = (float)(((cam.P[8] * X + cam.P[9] * Y) + cam.P[10] * Z) + cam.P[11]);
  osrc[k] = i;
}

}  // namespace
