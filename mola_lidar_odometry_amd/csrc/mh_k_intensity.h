// mh_k_intensity.h -- FilterNormalizeIntensity and FilterByIntensity [U] on the device (included by mh_preprocess.hip after
// mh_k_curv.h; semantics in include/molahip.h at mh_scan_normalize_intensity / mh_scan_by_intensity).
//   normalize: a min / max reduction over the layer's non-NaN intensities, then an in-place affine rewrite.
//   by-intensity: a classify kernel that writes the packed class word of mh_k_curv.h; the scan of those words, the
//   scatter (k_curv_scatter) and the read-back of the three counts are the curvature filter's own.
#pragma once

namespace {

__device__ __forceinline__ uint32_t int_ord(float f) {  // order-preserving (-0 < +0; NaNs are filtered out before)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float int_unord(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(u);
}

// words[0] = max over the values of ~ord(I) (= ~ord(min I)), words[1] = max of ord(I): both start at 0 (one hipMemsetAsync),
// and no non-NaN value encodes to 0 either way, so 0 / 0 means "no value".  Max is exact in any order: the result is the
// same bits whatever order the workgroups arrive in.  Grid-stride over a fixed grid with float4 loads (the channel starts a
// 256-byte aligned buffer); one shuffle reduction per wave, one LDS step across the four waves, one atomic pair per workgroup.
__global__ __launch_bounds__(256) void k_int_minmax(const float* __restrict__ in, uint32_t n, uint32_t* __restrict__ words) {
  __shared__ uint32_t slo[4], shi[4];
  uint32_t lo = 0u, hi = 0u;  // (lo holds the complement)
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const uint32_t n4 = n / 4u;
  const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
  for (uint32_t q = tid; q < n4; q += stride) {
    const float4 v = in4[q];
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (!isnan(e[c])) {
        const uint32_t o = int_ord(e[c]);
        lo = max(lo, ~o);
        hi = max(hi, o);
      }
  }
  for (uint32_t k = 4u * n4 + tid; k < n; k += stride)
    if (!isnan(in[k])) {
      const uint32_t o = int_ord(in[k]);
      lo = max(lo, ~o);
      hi = max(hi, o);
    }
  for (int off = 32; off > 0; off >>= 1) {
    lo = max(lo, (uint32_t)__shfl_xor((int)lo, off));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, off));
  }
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = max(max(slo[0], slo[1]), max(slo[2], slo[3]));
    hi = max(max(shi[0], shi[1]), max(shi[2], shi[3]));
    if (hi) {
      atomicMax(&words[0], lo);
      atomicMax(&words[1], hi);
    }
  }
}

// I' = (I - lo) * k, with lo / hi the layer's range widened by the remembered one (NaN: none) and k = 1 / (hi - lo) when
// that is > 0, else 0.  Every lane derives the same lo / k from the two words; the first lane also leaves {lo, hi} in
// page-locked host memory.  No range at all (empty or all-NaN layer, nothing remembered): nothing changes.
__global__ __launch_bounds__(256) void k_int_apply(float* __restrict__ io, uint32_t n, const uint32_t* __restrict__ words,
                                                   float rem_lo, float rem_hi, float* __restrict__ host_range) {
  const uint32_t w_lo = words[0], w_hi = words[1];
  float lo = w_hi ? int_unord(~w_lo) : __builtin_nanf(""), hi = w_hi ? int_unord(w_hi) : __builtin_nanf("");
  if (!isnan(rem_lo) && (isnan(lo) || rem_lo < lo)) lo = rem_lo;
  if (!isnan(rem_hi) && (isnan(hi) || rem_hi > hi)) hi = rem_hi;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid == 0) {
    host_range[0] = lo;
    host_range[1] = hi;
  }
  if (isnan(lo) && isnan(hi)) return;
  const float d = hi - lo;
  const float k = d > 0.f ? 1.0f / d : 0.0f;  // (HIP's default fp32 divide is correctly rounded)
  const uint32_t n4 = n / 4u;
  if (tid < n4) {
    float4* io4 = reinterpret_cast<float4*>(io);
    float4 v = io4[tid];
    v.x = (v.x - lo) * k;
    v.y = (v.y - lo) * k;
    v.z = (v.z - lo) * k;
    v.w = (v.w - lo) * k;
    io4[tid] = v;
  } else if (tid - n4 < n - 4u * n4) {  // the last n % 4 values
    const uint32_t q = 4u * n4 + (tid - n4);
    io[q] = (io[q] - lo) * k;
  }
}

// FilterByIntensity: the packed class word of mh_k_curv.h -- I < low -> low (field 0), else I > high -> high (field 2),
// else mid (field 1; NaN compares false both times).  Zero for the padding up to `cap`.
__global__ __launch_bounds__(256) void k_int_classify(const float* __restrict__ in, uint32_t n, uint32_t cap, float low,
                                                      float high, unsigned long long* __restrict__ word) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= cap) return;
  uint32_t f = 3u;  // none
  if (q < n) {
    const float v = in[q];
    f = v < low ? 0u : v > high ? 2u : 1u;
  }
  word[q] = f < 3u ? 1ull << (kCurvFieldBits * f) : 0ull;
}

}  // namespace
