// mh_k_frame_src.h -- what every kernel over a pass of posed key-frames shares (k_compose_frames, k_occf_rays, k_elev_points): the
// table entry of a frame, the search of a lane for its frame, and the composition of a point with its frame's pose.  No kernel
// lives here, so a translation unit that includes it gets no device code it does not launch.
#pragma once
#include <stdint.h>

namespace {

struct FrameSrc {
  const float *x, *y, *z;  // the frame's points (device memory; never read for an empty frame)
  double T[12];            // row-major 3x4, the key-frame's pose
};
static_assert(sizeof(FrameSrc) == 120, "FrameSrc is mirrored on the host byte for byte");

// the frame of point q: the last f in [lo, hi] with start[f] <= q (start[lo] <= q < start[hi + 1]); empty frames, whose
// offset equals their successor's, are stepped over by the upper bound
__device__ __forceinline__ uint32_t frame_of(const uint32_t* __restrict__ start, uint32_t lo, uint32_t hi, uint32_t q) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (start[mid] <= q) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// p_map = (float)(R*p + t) for point j of the frame, the arithmetic of k_compose_new (fp64, un-fused, rounded once).  FramePtr: the
// table entry -- FrameSrc or a structure that begins like it -- through the constant address space (a wave-uniform entry: scalar
// loads) or the global one (a lane's own entry).
template <class FramePtr>
__device__ __forceinline__ void compose_posed_point(FramePtr s, size_t j, float& ox, float& oy, float& oz) {
  const double px = ((const float __attribute__((address_space(1)))*)s->x)[j], py = ((const float __attribute__((address_space(1)))*)s->y)[j],
               pz = ((const float __attribute__((address_space(1)))*)s->z)[j];
  ox = (float)(((s->T[0] * px + s->T[1] * py) + s->T[2] * pz) + s->T[3]);
  oy = (float)(((s->T[4] * px + s->T[5] * py) + s->T[6] * pz) + s->T[7]);
  oz = (float)(((s->T[8] * px + s->T[9] * py) + s->T[10] * pz) + s->T[11]);
}

}  // namespace
