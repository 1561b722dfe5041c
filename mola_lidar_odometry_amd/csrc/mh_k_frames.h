// mh_k_frames.h -- the new points of a whole group of key-frames composed with their poses in one launch (included by
// mh_map.hip; semantics in include/molahip.h at mh_map_insert_frames).  What K calls of mh_map_insert do with K launches of
// k_compose_new, each followed by a rebuild of everything stored, is here ONE launch per pass followed by one rebuild:
//   k_compose_frames: one lane per new point of the pass.  The pass's frames lie behind one another in the numbering of its
//                     points; `start` is their prefix array (start[f] = first point of frame f, start[n_frames] = the total;
//                     an empty frame repeats an offset), `fr` the table of their arrays and poses.  Both live in device
//                     memory, not in the kernel arguments: their length is the caller's, and a lane indexes them with ITS frame.
// A wave first finds the frames of its first and of its last point with wave-uniform upper-bound searches (scalar loads).
// Where they agree -- ten thousand points per frame: all but one wave in 150 -- pose and array pointers are read once per
// wave through uniform addresses; a wave that straddles frames repeats the search per lane between those two bounds and
// reads its frame's entry per lane, as k_merge_fill does.  No LDS, no atomics, nothing shared between workgroups.
#pragma once

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

// p_map = (float)(R*p + t), the arithmetic of k_compose_new (fp64, un-fused, rounded once).  FramePtr: the table entry through
// the constant address space (a wave-uniform entry: scalar loads) or the global one (a lane's own entry).
#define MH_FRAMES_AS(n) __attribute__((address_space(n)))
template <class FramePtr>
__device__ __forceinline__ void compose_frame_point(FramePtr s, uint32_t j, uint32_t o, uint32_t src, float* __restrict__ ox,
                                                    float* __restrict__ oy, float* __restrict__ oz, uint32_t* __restrict__ osrc) {
  const double px = ((const float MH_FRAMES_AS(1)*)s->x)[j], py = ((const float MH_FRAMES_AS(1)*)s->y)[j],
               pz = ((const float MH_FRAMES_AS(1)*)s->z)[j];
  ox[o] = (float)(((s->T[0] * px + s->T[1] * py) + s->T[2] * pz) + s->T[3]);
  oy[o] = (float)(((s->T[4] * px + s->T[5] * py) + s->T[6] * pz) + s->T[7]);
  oz[o] = (float)(((s->T[8] * px + s->T[9] * py) + s->T[10] * pz) + s->T[11]);
  osrc[o] = src;
}

__global__ __launch_bounds__(256) void k_compose_frames(const uint32_t* __restrict__ start, const FrameSrc* __restrict__ fr,
                                                        uint32_t n_frames, uint32_t total, uint32_t src0, uint32_t n_old,
                                                        float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                        uint32_t* __restrict__ osrc) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  const uint32_t q_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q & ~63u));  // (wave-uniform)
  if (q_first >= total) return;
  const uint32_t q_last = min(q_first + 63u, total - 1u);
  const uint32_t f_first = frame_of(start, 0u, n_frames - 1u, q_first);
  const uint32_t f_last = frame_of(start, f_first, n_frames - 1u, q_last);
  if (q >= total) return;
  if (f_first == f_last) {  // (wave-uniform branch)
    compose_frame_point((const FrameSrc MH_FRAMES_AS(4)*)(fr + f_first), q - start[f_first], n_old + q, src0 + q, ox, oy, oz, osrc);
  } else {
    const uint32_t f = frame_of(start, f_first, f_last, q);
    compose_frame_point((const FrameSrc MH_FRAMES_AS(1)*)(fr + f), q - start[f], n_old + q, src0 + q, ox, oy, oz, osrc);
  }
}

#undef MH_FRAMES_AS

}  // namespace
