/* molahip_nav.h -- an inflated costmap, the clearance and the reachable region over a 2-D cost plane: the seventh public header of
 * libmolahip.so.  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is, this
 * surface has a version of its own.  Conventions (status codes, `mem` spaces, streams, ownership) are molahip.h's.
 *
 * An mh_nav is a window of nx * ny cells, ny * nx entries per plane, y outer (entry [r * nx + c] is the cell in column c of row r).
 * It holds four planes:
 *     base   uint8   what the caller gives: 255 unknown, 254 lethal, 0..253 a cost
 *     d2     uint16  the squared distance, in cells, to the nearest obstacle cell; MH_NAV_FAR where none lies within max_cells
 *     cost   uint8   the inflated cost, in the byte convention of `base`
 *     reach  uint8   1 where the cell can be reached from a seed, 0 elsewhere
 * Everything is integer: results are exact and depend neither on thread order nor on how the work is split into tiles or sweeps.
 *
 * mh_nav_create.  MH_ERR_INVALID_ARGUMENT: a NULL argument; nx or ny of 0; nx * ny > 2^26.  No plane is valid yet.
 *
 * mh_nav_set_base -- `bytes` is an array of ny * nx uint8 in the memory space `mem` (MH_MEM_HOST, MH_MEM_DEVICE or
 *   MH_MEM_HOST_PINNED).  It replaces `base` and invalidates d2, cost and reach.  The call is synchronous: on return the caller's
 *   array may be reused.
 *
 * mh_nav_inflate(nav, max_cells, unknown_is_obstacle, table, n_table) -- with R = max_cells, 0 <= R <= MH_NAV_MAX_CELLS (255).
 *   `table` is a HOST array of n_table = R * R + 1 bytes, every entry <= MH_NAV_MAX_TABLE (253): inflation can never make a lethal
 *   or an unknown cell.  table[0] is never read.
 *   OBSTACLE.  A cell is an obstacle when base == 254, or when unknown_is_obstacle != 0 and base == 255.
 *   d2[c] = the minimum over the obstacle cells o of the window of (cx - ox)^2 + (cy - oy)^2; when that minimum exceeds R * R, or
 *   the window holds no obstacle, d2[c] = MH_NAV_FAR (65535).  (An obstacle cell itself has d2 = 0.)
 *   cost[c] = 255 where base[c] == 255;  254 where base[c] == 254;  otherwise max(base[c], d2[c] == MH_NAV_FAR ? 0 : table[d2[c]]).
 *   It validates d2 and cost and invalidates reach.
 *   (Shape: a column pass writes the vertical distance to the nearest obstacle within R, or none; a row pass takes the minimum of
 *   g(x + dx)^2 + dx^2 over |dx| <= R from a row segment staged with its halo in LDS.  No atomics, nothing is read back.  From a
 *   window with nx >= MH_NAV_ROW_SEGMENT the row pass works in segments of MH_NAV_ROW_SEGMENT cells; from a window with nx and ny
 *   >= MH_NAV_COL_TILE the column pass works in tiles of MH_NAV_COL_TILE x MH_NAV_COL_TILE cells; narrower windows get narrower,
 *   taller tiles.  The results do not depend on any of this.)
 *
 * mh_nav_reach(nav, seeds_xy, n_seeds, passable_below) -- `seeds_xy` is a HOST array of n_seeds (column, row) pairs of int32,
 *   relative to the window (it may be NULL when n_seeds == 0).  passable_below lies in 1 .. 254.
 *   PASSABLE.  A cell is passable iff cost < passable_below.
 *   reach[c] = 1 iff c is passable and a 4-connected path of passable cells joins it to a seed that stands on a passable cell;
 *   0 otherwise.  Cells that touch only diagonally are not joined.  The result is the union of the components of passable cells that
 *   hold a seed: it does not depend on the order of the seeds.  n_seeds == 0 gives an all-zero plane.
 *   A seed outside the window (column not in [0, nx) or row not in [0, ny)) is ignored and counted in n_seeds_outside; a seed on an
 *   impassable cell marks nothing and is counted in n_seeds_blocked (each seed counts, also when several name one cell).
 *   (Shape: a tile with its one-cell halo relaxes in LDS until it stops changing, writes back and raises one flag when it changed a
 *   cell; the HOST repeats such sweeps until one changes nothing.  n_sweeps = the sweeps launched, the last of which changed
 *   nothing; 0 when no seed stands on a passable cell.  No workgroup waits for another.  From a window with nx >= MH_NAV_REACH_TILE_X
 *   and ny >= MH_NAV_REACH_TILE_Y the tiles are MH_NAV_REACH_TILE_X x MH_NAV_REACH_TILE_Y cells.)
 *   MH_ERR_INVALID_ARGUMENT when cost is not valid (no mh_nav_inflate since the last mh_nav_set_base).
 *
 * mh_nav_download(nav, d2, cost, reach) -- to HOST arrays of ny * nx entries; any of the three may be NULL.
 *   MH_ERR_INVALID_ARGUMENT, nothing copied: a plane is asked for that has not been computed since the last mh_nav_set_base.
 *
 * Refusals.  MH_ERR_INVALID_ARGUMENT before any device work, the handle untouched: a NULL argument (table and, with n_seeds > 0,
 * seeds_xy included); a bad `mem`; max_cells > 255; n_table != max_cells^2 + 1; a table entry > 253; mh_nav_inflate before
 * mh_nav_set_base; passable_below outside 1 .. 254.
 *
 * NOT BUILT: footprints other than a disc; 8-connectivity; a distance beyond 255 cells; incremental use while driving (every call
 * works on the whole window); several devices.  (A cost-to-go field and routes over the cost plane: include/molahip_plan.h.)
 *
 * Threads.  As every handle of the library, an mh_nav is not to be used by two calls at once; mh_nav_download and mh_nav_get_info
 * take a const handle because they leave the planes alone. */
#ifndef MOLAHIP_NAV_H_
#define MOLAHIP_NAV_H_

#include "molahip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_NAV_API_VERSION 1
#define MH_NAV_FAR 65535
#define MH_NAV_MAX_CELLS 255
#define MH_NAV_MAX_TABLE 253
#define MH_NAV_UNKNOWN 255
#define MH_NAV_LETHAL 254
#define MH_NAV_ROW_SEGMENT 256
#define MH_NAV_COL_TILE 64
#define MH_NAV_REACH_TILE_X 64
#define MH_NAV_REACH_TILE_Y 16

typedef struct mh_nav mh_nav;
typedef struct {
  uint32_t nx, ny;          /* columns, rows */
  uint32_t has_base;        /* 1 after mh_nav_set_base */
  uint32_t has_cost;        /* 1 when d2 and cost have been computed since the last mh_nav_set_base */
  uint32_t has_reach;       /* ... and reach */
  uint32_t max_cells;       /* R of the last mh_nav_inflate */
  uint32_t n_sweeps;        /* of the last mh_nav_reach */
  uint32_t reserved_;
  uint64_t n_reached;       /* cells with reach == 1 */
  uint64_t n_seeds_blocked; /* seeds inside the window on impassable cells */
  uint64_t n_seeds_outside; /* seeds outside the window */
} mh_nav_info;              /* 56 bytes */

/* MH_NAV_API_VERSION of the loaded library. */
MH_API uint32_t mh_nav_api_version(void);
MH_API mh_status mh_nav_create(mh_ctx* ctx, uint32_t nx, uint32_t ny, mh_nav** out);
MH_API mh_status mh_nav_destroy(mh_nav* nav);
MH_API mh_status mh_nav_get_info(const mh_nav* nav, mh_nav_info* info);
MH_API mh_status mh_nav_set_base(mh_nav* nav, const uint8_t* bytes, int32_t mem);
MH_API mh_status mh_nav_inflate(mh_nav* nav, uint32_t max_cells, int32_t unknown_is_obstacle, const uint8_t* table, size_t n_table);
MH_API mh_status mh_nav_reach(mh_nav* nav, const int32_t* seeds_xy, size_t n_seeds, uint32_t passable_below);
MH_API mh_status mh_nav_download(const mh_nav* nav, uint16_t* d2, uint8_t* cost, uint8_t* reach);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_NAV_H_ */
