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
#include "mh_k_frame_src.h"  // FrameSrc, frame_of, compose_posed_point

namespace {

#define MH_FRAMES_AS(n) __attribute__((address_space(n)))
template <class FramePtr>
__device__ __forceinline__ void compose_frame_point(FramePtr s, uint32_t j, uint32_t o, uint32_t src, float* __restrict__ ox,
                                                    float* __restrict__ oy, float* __restrict__ oz, uint32_t* __restrict__ osrc) {
  float px, py, pz;
  compose_posed_point(s, j, px, py, pz);
  ox[o] = px;
  oy[o] = py;
  oz[o] = pz;
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
