/* molahip_occgrid.h -- a navigation occupancy grid from recorded key-frames: the fourth public header of libmolahip.so
 * (DESIGN.md row g12).  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is, this surface
 * has a version of its own.  Conventions (status codes, `mem` spaces, streams, ownership) are molahip.h's; the occupancy map,
 * its cells, its five log-odds integers and the insert rule (steps 1 to 6) are those written down at mh_occmap_insert there.
 *
 * Every key-frame of a recorded session is a scan with a pose.  Ray-traced into an mh_occmap, the key-frames carry free-space
 * evidence as well as obstacles; a height band of the resulting cells, projected along z, is the 2-D raster that navigation
 * stacks load.  Everything here is integer: results are exact and depend neither on thread order nor on how the work is split.
 *
 * mh_occmap_insert_frames -- a whole group of key-frames ray-traced into the map at once.
 *  - DEFINITION.  Afterwards the map is bit for bit the map after
 *        for f in 0 .. n_frames-1:  mh_occmap_insert(occ, scan(frames[f]), frames[f].T, 0)
 *    -- the same mh_occmap_download (keys and log-odds), the same n_cells / n_occupied, the same centres in the same order in
 *    the search map and the same current V, the same result of a following mh_occmap_insert or mh_occmap_insert_frames.  There
 *    is no far removal.  (K single inserts sort, merge-join the whole store, rebuild the search map and read counters back K
 *    times; this call does each once per pass and rebuilds the search map once.)
 *  - mh_occmap_info afterwards: n_left_out and n_keys are the CALL's totals (the sums of what the K single inserts would each
 *    report); n_passes is the number of key chunks the call worked (below), summed over its passes.
 *  - Order matters.  Step 5 of the insert rule clamps per insert, so frames do not commute on a cell: a cell at l_max that frame
 *    A looks through and frame B then hits ends at l_max again, while the summed counts (one hit, one miss applied in one insert:
 *    hits first) end at l_max - l_miss.  The counts therefore stay per (cell, frame) and are folded per cell in frame order, each
 *    frame applying its own rule: MH_OCC_COUNTED: hits, clamp, then misses, clamp;  MH_OCC_ONCE: hit, else miss.
 *  - Passes.  Frames are taken in order into passes of at most max_points_per_pass points (0: the library's default, 2^21);
 *    a frame larger than that is a pass of its own.  Inside a pass more than mh_occmap_params::max_keys_per_pass keys are worked
 *    in chunks whose per-(cell, frame) counts are summed before the fold.  The result depends on neither size; small values
 *    exist for tests.  Passes are sequential updates of the store, which the definition allows.
 *  - The search map is rebuilt once, at the end of the call.  A failure in a later pass (out of memory) leaves the earlier
 *    passes applied and the handle usable: the store, n_cells / n_occupied and the search map are those after the last completed
 *    pass, and n_left_out / n_keys / n_passes of mh_occmap_get_info are the totals of the completed passes.
 *  - Arrays live in `mem`: MH_MEM_HOST, MH_MEM_HOST_PINNED or MH_MEM_DEVICE (device arrays are read in place; x, y, z of a frame
 *    may be NULL when its n is 0).  The call is synchronous: on return the caller's arrays may be reused.
 *  - MH_ERR_INVALID_ARGUMENT before any device work, the map untouched: a NULL map; NULL frames with n_frames > 0; a bad `mem`;
 *    NULL arrays with n > 0; a non-finite pose entry (of an empty frame too); a pose whose translation lies outside the key range
 *    (mh_occmap_insert's refusal, here for the call as a whole); n_frames > MH_MAX_INSERT_FRAMES; a frame of 0x7FFFFFF0 points or
 *    more.  Whether device arrays belong to the map's context cannot be told from a pointer and is not checked.
 *  - n_frames == 0 or only empty frames: MH_OK, nothing changes (the info of the last insert included).
 *
 * mh_occmap_index_bounds -- the per-axis minimum lo[3] and maximum hi[3] of the cell indices over the stored cells (an integer
 *    reduction on the device) and their number.  On an empty map *n_cells = 0 and lo / hi are left untouched.
 *
 * mh_occmap_project_grid -- the stored cells of a height band projected along z.
 *  - mh_occgrid_window holds integers only: x0, y0 = the cell index of grid column 0 and of grid row 0; nx, ny = columns and
 *    rows; z_lo, z_hi = the inclusive cell indices of the band.
 *  - max_logodds is a HOST array of ny * nx int32, row-major with y outer: entry [r * nx + c] is the maximum log-odds over the
 *    stored cells (x0 + c, y0 + r, z) with z_lo <= z <= z_hi, and INT32_MIN (MH_OCCGRID_NONE) where the band holds no stored
 *    cell.  One lane per stored cell, an integer maximum: exact and independent of order.
 *  - MH_ERR_INVALID_ARGUMENT: a NULL argument, nx or ny of 0, nx * ny > 2^28, z_lo > z_hi.
 *
 * Threads.  As every call on an mh_occmap, the three calls are not to run concurrently on one handle: mh_occmap_index_bounds and
 * mh_occmap_project_grid take a const handle because they leave the map's content alone, but they use the handle's scratch and read-back
 * words.
 *
 * The trinary rule of a grid (a pure host rule; mola_hip::OccupancyGrid and tests/occgrid_ref.py restate it): a cell is UNKNOWN
 * where the maximum is MH_OCCGRID_NONE, OCCUPIED where the maximum is >= l_occ (mh_occmap_info), FREE otherwise.
 * A height z [m] becomes a cell index by the floor rule of the map in fp64: floor(z * (1 / resolution)), with 1 / resolution the
 * fp32 reciprocal the map itself uses, widened. */
#ifndef MOLAHIP_OCCGRID_H_
#define MOLAHIP_OCCGRID_H_

#include "molahip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_OCCGRID_API_VERSION 1
#define MH_OCCGRID_NONE INT32_MIN

typedef struct {
  int32_t x0, y0;     /* cell index of grid column 0 / row 0 */
  uint32_t nx, ny;    /* columns, rows; nx * ny <= 2^28 */
  int32_t z_lo, z_hi; /* inclusive cell indices of the height band */
} mh_occgrid_window;  /* 24 bytes */

/* MH_OCCGRID_API_VERSION of the loaded library. */
MH_API uint32_t mh_occgrid_api_version(void);
MH_API mh_status mh_occmap_insert_frames(mh_occmap* occ, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                         uint64_t max_points_per_pass);
MH_API mh_status mh_occmap_index_bounds(const mh_occmap* occ, int32_t lo[3], int32_t hi[3], uint64_t* n_cells);
MH_API mh_status mh_occmap_project_grid(const mh_occmap* occ, const mh_occgrid_window* window, int32_t* max_logodds);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_OCCGRID_H_ */
