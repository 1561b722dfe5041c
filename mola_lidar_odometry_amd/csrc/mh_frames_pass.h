// mh_frames_pass.h -- what every batched posed-frame call over mh_map_frame shares on the host (mh_map_insert_frames,
// mh_occmap_insert_frames, the point passes of molahip_elevation.h): the refusals, the split of the frames into passes, and one
// pass's upload.  The reading is written down in include/molahip.h at mh_map_insert_frames; the device side of it (FrameSrc, the
// upper-bound search of a lane for its frame, the composition of a point with its pose) is mh_k_frame_src.h's.
#pragma once
#include <math.h>
#include <string.h>

#include "mh_internal.h"

namespace mh {

// The library's own pass size (max_points_per_pass == 0): 2 M points are 24 MB of staged coordinates.
constexpr uint64_t kFramesPassPoints = 1ull << 21;

// The refusals before any device work, reported under the entry point's name `fn`; *sum = the points of the whole call.
inline mh_status frames_check(const char* fn, const mh_map_frame* frames, size_t n_frames, int32_t mem, uint64_t* sum) {
  auto refuse = [&](const char* msg) { return fail(MH_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg); };
  if (!(n_frames == 0 || frames)) return refuse("null frames");
  if (!(mem == MH_MEM_HOST || mem == MH_MEM_DEVICE || mem == MH_MEM_HOST_PINNED)) return refuse("bad mem space");
  if (!(n_frames <= MH_MAX_INSERT_FRAMES)) return refuse("too many frames");
  *sum = 0;
  for (size_t f = 0; f < n_frames; f++) {
    const mh_map_frame& fr = frames[f];
    if (!(fr.n == 0 || (fr.x && fr.y && fr.z))) return refuse("null point arrays");
    if (!(fr.n < 0x7FFFFFF0ull)) return refuse("too many points");
    for (int i = 0; i < 12; i++)
      if (!isfinite(fr.T[i])) return refuse("non-finite pose");
    *sum += fr.n;  // (2^20 frames of less than 2^31 points: no overflow)
  }
  return MH_OK;
}

// The pass that starts at frame f0: frames in order while they fit the budget; a frame larger than it is a pass of its own.
// Returns the frame behind the pass; *P = the pass's points (0: only empty frames were left).
inline size_t frames_next_pass(const mh_map_frame* frames, size_t n_frames, size_t f0, uint64_t budget, uint64_t* P) {
  size_t f1 = f0;
  *P = 0;
  while (f1 < n_frames && (*P == 0 || *P + frames[f1].n <= budget)) *P += frames[f1++].n;
  return f1;
}

// One pass's upload: [x | y | z of the pass's points (host arrays only)] prefix array [nf + 1] | frame table [nf]
struct FramesUpload {
  size_t pstride, off_start, off_table, bytes;
};
inline size_t frames_up256(size_t b) { return ((b + 255) / 256) * 256; }
inline FramesUpload frames_upload_layout(size_t nf, uint64_t P, bool staged, size_t entry_bytes) {
  FramesUpload u;
  u.pstride = staged ? frames_up256(P * sizeof(float)) : 0;
  u.off_start = 3 * u.pstride;
  u.off_table = u.off_start + frames_up256((nf + 1) * sizeof(uint32_t));
  u.bytes = u.off_table + nf * entry_bytes;
  return u;
}
// Fills the mirror `h` (u.bytes) of the block that will lie at device address `d`: host arrays are packed into it, device arrays
// are named in place.  Entry: a table entry that begins with x, y, z and T[12] (FrameSrc, OccFrame); the prefix array written here
// is over all points (a caller that selects points writes its own over it).
template <class Entry>
inline void frames_fill_upload(const FramesUpload& u, const mh_map_frame* frames, size_t nf, bool staged, char* h, char* d) {
  uint32_t* h_start = (uint32_t*)(h + u.off_start);
  Entry* h_tab = (Entry*)(h + u.off_table);
  uint64_t at = 0;
  for (size_t k = 0; k < nf; k++) {
    const mh_map_frame& fr = frames[k];
    h_start[k] = (uint32_t)at;
    Entry& e = h_tab[k];
    if (staged) {
      if (fr.n) {
        memcpy(h + at * sizeof(float), fr.x, fr.n * sizeof(float));
        memcpy(h + u.pstride + at * sizeof(float), fr.y, fr.n * sizeof(float));
        memcpy(h + 2 * u.pstride + at * sizeof(float), fr.z, fr.n * sizeof(float));
      }
      e.x = (const float*)d + at;
      e.y = (const float*)(d + u.pstride) + at;
      e.z = (const float*)(d + 2 * u.pstride) + at;
    } else {
      e.x = fr.x; e.y = fr.y; e.z = fr.z;
    }
    for (int i = 0; i < 12; i++) e.T[i] = fr.T[i];
    at += fr.n;
  }
  h_start[nf] = (uint32_t)at;
}

}  // namespace mh
