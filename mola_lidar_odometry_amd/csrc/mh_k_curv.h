// mh_k_curv.h -- FilterCurvature [U] on the device (included by mh_preprocess.hip; semantics in include/molahip.h at
// mh_scan_curvature): a three-point stencil that sorts every interior point into one of three classes, then an ordered
// three-way compaction.  Same flag -> position -> compact shape as k_pp_flag_b / k_pp_compact_b, with ONE scan for the three
// outputs: each point contributes a 64-bit word holding a 1 in the 21-bit field of its class, so the exclusive scan of
// those words gives every point its place in its own output, and the scan's total gives the three counts.
#pragma once

namespace {

constexpr uint32_t kCurvFieldBits = 21;                                // three counters in one uint64
constexpr size_t kCurvMaxPoints = (size_t(1) << kCurvFieldBits) - 1;  // a field may not overflow into the next
enum : uint32_t { kCurvNone = 0, kCurvLarger = 1, kCurvSmaller = 2, kCurvOther = 3 };

// word[i] = 1 << (21 * (class - 1)), 0 for the two end points (and the padding up to `cap`, which the scan runs over)
__global__ __launch_bounds__(256) void k_curv_classify(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, uint32_t n, uint32_t cap,
                                                       float max_cosine, float clr2, float gap2,
                                                       unsigned long long* __restrict__ word) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  uint32_t cls = kCurvNone;
  if (i >= 1u && i + 1u < n) {
    const float px = x[i - 1], py = y[i - 1], pz = z[i - 1];
    const float cx = x[i], cy = y[i], cz = z[i];
    const float qx = x[i + 1], qy = y[i + 1], qz = z[i + 1];
    const float ax = cx - px, ay = cy - py, az = cz - pz;
    const float bx = qx - cx, by = qy - cy, bz = qz - cz;
    const float na = (ax * ax + ay * ay) + az * az;
    const float nb = (bx * bx + by * by) + bz * bz;
    if (na > gap2 || nb > gap2) {
      cls = kCurvOther;
    } else if (na < clr2 || nb < clr2) {
      cls = kCurvOther;
    } else {
      // (-ffp-contract=off and HIP's default correctly rounded fp32 divide and square root: the restatement's own ops)
      const float c = ((ax * bx + ay * by) + az * bz) / (sqrtf(na) * sqrtf(nb));
      cls = c < max_cosine ? kCurvLarger : kCurvSmaller;  // (NaN compares false: smaller, as specified)
    }
  }
  word[i] = cls ? 1ull << (kCurvFieldBits * (cls - 1u)) : 0ull;
}

struct CurvOut {
  float *x, *y, *z, *t;  // t null: no time stamps (the input has none)
  float* i;              // null: no intensity (the input has none)
  uint32_t* src;         // null: this output was not asked for
};

// scatter every classified point to its output (also the words of k_int_classify, mh_k_intensity.h); the first lane also writes the three counts (the scan's total) to
// page-locked host memory
__global__ __launch_bounds__(256) void k_curv_scatter(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ z, const float* __restrict__ t,
                                                      const float* __restrict__ in_i, const uint32_t* __restrict__ src,
                                                      uint32_t n, uint32_t cap,
                                                      const unsigned long long* __restrict__ word,
                                                      const unsigned long long* __restrict__ pos, CurvOut o0, CurvOut o1,
                                                      CurvOut o2, uint32_t* __restrict__ host_counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr unsigned long long kMask = (1ull << kCurvFieldBits) - 1ull;
  if (i == 0) {
    const unsigned long long total = pos[cap - 1] + word[cap - 1];
    host_counts[0] = (uint32_t)(total & kMask);
    host_counts[1] = (uint32_t)((total >> kCurvFieldBits) & kMask);
    host_counts[2] = (uint32_t)((total >> (2 * kCurvFieldBits)) & kMask);
  }
  if (i >= n) return;
  const unsigned long long w = word[i];
  if (!w) return;
  const uint32_t f = w == 1ull ? 0u : w == (1ull << kCurvFieldBits) ? 1u : 2u;
  // (the output picked field by field with selects: a reference into the kernel's arguments would live in scratch)
  uint32_t* osrc = f == 0u ? o0.src : f == 1u ? o1.src : o2.src;
  if (!osrc) return;
  float* ox = f == 0u ? o0.x : f == 1u ? o1.x : o2.x;
  float* oy = f == 0u ? o0.y : f == 1u ? o1.y : o2.y;
  float* oz = f == 0u ? o0.z : f == 1u ? o1.z : o2.z;
  const uint32_t k = (uint32_t)((pos[i] >> (kCurvFieldBits * f)) & kMask);
  ox[k] = x[i];
  oy[k] = y[i];
  oz[k] = z[i];
  if (t) (f == 0u ? o0.t : f == 1u ? o1.t : o2.t)[k] = t[i];
  if (in_i) (f == 0u ? o0.i : f == 1u ? o1.i : o2.i)[k] = in_i[i];
  osrc[k] = src ? src[i] : i;
}

}  // namespace
