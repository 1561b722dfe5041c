// mh_flat_off32.h -- the size rule behind the plan / scan matcher's two instantiations (k_match_flat<OFF32>, k_match_flat_b<OFF32>,
// mh_k_launch.h).  Plain C++, no HIP header: tests/test_flat_off32_cpu.py compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mh {

// May a launch form the byte offsets of its gathers in 32 bits (gat<true>, mh_nn_device.h)?  `slots_bytes`, `pts_bytes` and
// `pts_q_bytes` are the sizes of the map's three allocations, `scan_points` the scan's length.
//
// The argument: gat<true>(base, i) computes i * sizeof(T) in 32 bits and zero-extends it, which is the byte offset of element i
// exactly when that product is below 2^32.  For every array the kernels address that way the largest index is below the element
// count, so the largest byte offset is at most bytes - sizeof(T), which is below 2^32 when bytes <= 2^32:
//   slots       16-byte slots; index = hash & mask and its linear-probing successors (h + 1) & mask, all < table_size, and the
//               allocation holds table_size slots;
//   pts         16-byte records; index = a record number the search found (< n_points <= pts' records);
//   pts_q       16-byte records; index = first + j with j < the slot's count, clamped into the chunk / the merged ranges
//               (flat_plan_scan phase B, nn_scan_round_quad): inside the voxel's records;
//   lx, ly, lz  4 bytes per scan point, index = min(i, n - 1) < n:                        offset <= 4 n - 4;
//   pair_q      16 bytes per scan point, the same index (and i0 + p < n in phase D):      offset <= 16 n - 16;
//   pair_gidx   4 bytes per scan point, the same indices:                                 offset <= 4 n - 4;
// the scan's arrays are bounded through the point count (16 n <= 2^32 covers all three widths), not through the sizes of the
// grow-only buffers they live in.  Conservative: a grow-only map buffer that is larger than its content only sends the launch to
// the 64-bit instantiation.  (`scan_points` is compared, not multiplied: no count wraps.)
inline bool flat_off32_sizes(uint64_t slots_bytes, uint64_t pts_bytes, uint64_t pts_q_bytes, uint64_t scan_points) {
  constexpr uint64_t kLim = (uint64_t)1 << 32;
  return slots_bytes <= kLim && pts_bytes <= kLim && pts_q_bytes <= kLim && scan_points <= kLim / 16u;
}

}  // namespace mh
