/* molahip_plan.h -- a cost-to-go field over a 2-D cost plane and routes traced down it: the eighth public header of libmolahip.so
 * (DESIGN.md row g16).  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is, this surface has a
 * version of its own.  Conventions (status codes, `mem` spaces, streams, ownership) are molahip.h's.
 *
 * An mh_plan is a window of nx * ny cells, ny * nx entries per plane, y outer (entry [r * nx + c] is the cell in column c of row r).
 * It holds two planes:
 *     cost   uint8   what the caller gives, in the byte convention of mh_nav's cost plane: 255 unknown, 254 lethal, 0..253 a cost
 *     field  uint32  the cost-to-go: the length of the cheapest route to the nearest goal; MH_PLAN_UNREACHED (0xFFFFFFFF) where the
 *                    cell is impassable or not joined to a goal
 * Everything is integer: results are exact and depend neither on thread order nor on how the work is split into tiles or sweeps.
 *
 * mh_plan_create.  MH_ERR_INVALID_ARGUMENT: a NULL argument; nx or ny of 0; nx * ny > 2^26.  No plane is valid yet.
 *
 * mh_plan_set_cost -- `bytes` is an array of ny * nx uint8 in the memory space `mem` (MH_MEM_HOST, MH_MEM_DEVICE or
 *   MH_MEM_HOST_PINNED).  It replaces `cost` and invalidates the field.  The call is synchronous: on return the caller's array may be
 *   reused.
 *
 * mh_plan_set_cost_from_nav(plan, nav) -- the same from the cost plane of an mh_nav (include/molahip_nav.h), device to device.
 *   MH_ERR_INVALID_ARGUMENT, the handle untouched: `nav` has no valid cost (no mh_nav_inflate since its last mh_nav_set_base), its nx
 *   or ny differ from the plan's, or it was created on another context.
 *
 * mh_plan_field(plan, goals_xy, n_goals, passable_below, price, n_price)
 *   THE FIELD RULE.
 *   passable_below lies in 1 .. 254.  `price` is a HOST array of n_price == passable_below uint16 values, every entry >= 1.
 *   PASSABLE.  A cell c is passable iff cost[c] < passable_below.  Its price is p(c) = price[cost[c]].
 *   STEPS.  From a passable cell there is a step to each of its 8 neighbours that lies inside the window and is passable; a diagonal
 *   step exists only when both cells it passes between are passable as well (for the step (x, y) -> (x + 1, y + 1) those are
 *   (x + 1, y) and (x, y + 1)).  No corner is cut, so the cells with a finite field are exactly the cells mh_nav_reach marks for the
 *   same seeds and the same passable_below.
 *   STEP WEIGHT.  w(a, b) = L * (p(a) + p(b)) with L = 5 for an orthogonal step and L = 7 for a diagonal one: 10 and 14 times the
 *   mean price of the two cells.  It is symmetric: the distance to a goal is the distance from it.
 *   FIELD.  field[c] = the minimum, over the goals g that stand on a passable cell and over the step paths from c to g, of the sum of
 *   the step weights; 0 on such a goal cell; MH_PLAN_UNREACHED where c is impassable or no such path exists.
 *   GOALS.  `goals_xy` is a HOST array of n_goals (column, row) pairs of int32, relative to the window (it may be NULL when n_goals
 *   == 0).  A goal outside the window (column not in [0, nx) or row not in [0, ny)) is ignored and counted in n_goals_outside; a goal
 *   on an impassable cell marks nothing and is counted in n_goals_blocked (each goal counts, also when several name one cell).  The
 *   order of the goals plays no part.  n_goals == 0, or no goal on a passable cell, gives an all-UNREACHED plane and n_sweeps == 0.
 *   NO WRAP-AROUND.  A shortest path visits a cell at most once, so every finite value is at most (nx * ny - 1) * 14 * max(price).
 *   The call is refused, before any device work, unless that bound -- computed in 64 bits over the n_price entries -- is below
 *   0xFFFFFFFF.  (A derived condition, not a tuned limit: a window of 4096 x 4096 admits prices up to 18, one of 1000 x 1000 up to
 *   306.)
 *   It validates the field.  max_field = the largest finite value (0 when there is none), n_reached = the cells with a finite value.
 *   (Shape: a tile with its one-cell halo relaxes every cell against its 8 neighbours in LDS until no lane lowers a value, writes
 *   back the cells it lowered and raises the sweep's flag; the HOST repeats such sweeps until one changes nothing.  n_sweeps = the
 *   sweeps launched, the last of which changed nothing.  A tile stages and relaxes only when it or one of its 8 neighbour tiles
 *   changed in the previous sweep -- in the first sweep the tiles that hold a goal and their 8 neighbours count as changed;
 *   n_tile_runs = the tiles that staged and relaxed, summed over the sweeps.  With MH_PLAN_ALL_TILES=1 in the environment, read per
 *   call, every tile runs in every sweep: for measuring only.  n_sweeps and n_tile_runs may differ from run to run; the planes do
 *   not.  No workgroup waits for another.  From a window with nx >= MH_PLAN_TILE_X and ny >= MH_PLAN_TILE_Y the tiles are
 *   MH_PLAN_TILE_X x MH_PLAN_TILE_Y cells; narrower or lower windows get narrower, taller or wider, lower tiles.  The results do not
 *   depend on any of this.)
 *   MH_ERR_INTERNAL when the sweeps do not come to rest within nx * ny of them (they always do).
 *
 * mh_plan_trace(plan, starts_xy, n_starts, cap, out_xy, out_len)
 *   THE TRACE RULE.  `starts_xy` is a HOST array of n_starts (column, row) pairs of int32 (it may be NULL when n_starts == 0).  Per
 *   start i:  out_len[i] = 0 when the start lies outside the window or its field is MH_PLAN_UNREACHED.  Otherwise the route is the
 *   sequence of cells c0 = the start, c1, ... that ends at the first cell with field 0, where c(k+1) is the neighbour n of ck, by a
 *   step the field rule allows, that minimises field[n] + w(ck, n) -- that minimum equals field[ck].  Ties go to the first in the
 *   order E, N, W, S, NE, NW, SW, SE, with E = column + 1 and N = row + 1.  The field strictly falls along the route, so it ends.
 *   `out_xy` is a HOST array of n_starts * cap (column, row) pairs of int32: route i begins at pair i * cap.  `out_len` is a HOST array
 *   of n_starts uint32: the number of cells of route i, its start and its end included.  When the route has more than `cap` cells the
 *   first `cap` are written and out_len[i] = MH_PLAN_TRUNCATED (0xFFFFFFFF).  Pairs beyond a route's length are left as they were.
 *   It needs a valid field and cap >= 1, and uses the passable_below and the prices of the mh_plan_field call that made the field.
 *
 * mh_plan_download(plan, field) -- to a HOST array of ny * nx uint32.  MH_ERR_INVALID_ARGUMENT, nothing copied, when no field is
 *   valid.
 *
 * Refusals.  MH_ERR_INVALID_ARGUMENT before any device work, the handle untouched: a NULL argument (price and, with n_goals > 0 or
 *   n_starts > 0, goals_xy or starts_xy, out_xy and out_len included); a bad `mem`; passable_below outside 1 .. 254; n_price !=
 *   passable_below; a price of 0; the wrap-around bound; mh_plan_field before a cost was set; mh_plan_trace or mh_plan_download before
 *   mh_plan_field; cap == 0.
 *
 * NOT BUILT: any-angle or kinematic routes; footprints other than a disc; several devices.  (Replanning while driving: every call here
 * works on the whole window; include/molahip_replan.h repairs the field after the cost of a rectangle of cells changed.)
 *
 * Threads.  As every handle of the library, an mh_plan is not to be used by two calls at once; mh_plan_trace, mh_plan_download and
 * mh_plan_get_info take a const handle where they leave the planes alone. */
#ifndef MOLAHIP_PLAN_H_
#define MOLAHIP_PLAN_H_

#include "molahip.h"
#include "molahip_nav.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_PLAN_API_VERSION 1
#define MH_PLAN_UNREACHED 0xFFFFFFFFu
#define MH_PLAN_TRUNCATED 0xFFFFFFFFu
#define MH_PLAN_TILE_X 64
#define MH_PLAN_TILE_Y 16
#define MH_PLAN_STEP_ORTHOGONAL 5
#define MH_PLAN_STEP_DIAGONAL 7

typedef struct mh_plan mh_plan;
typedef struct {
  uint32_t nx, ny;          /* columns, rows */
  uint32_t has_cost;        /* 1 after mh_plan_set_cost / mh_plan_set_cost_from_nav */
  uint32_t has_field;       /* 1 when the field has been computed since the cost was last set */
  uint32_t passable_below;  /* of the last mh_plan_field */
  uint32_t n_sweeps;        /* of the last mh_plan_field */
  uint32_t max_field;       /* the largest finite value of the field */
  uint32_t reserved_;
  uint64_t n_reached;       /* cells with a finite field */
  uint64_t n_goals_blocked; /* goals inside the window on impassable cells */
  uint64_t n_goals_outside; /* goals outside the window */
  uint64_t n_tile_runs;     /* tiles that staged and relaxed, over all sweeps */
} mh_plan_info;             /* 64 bytes */

/* MH_PLAN_API_VERSION of the loaded library. */
MH_API uint32_t mh_plan_api_version(void);
MH_API mh_status mh_plan_create(mh_ctx* ctx, uint32_t nx, uint32_t ny, mh_plan** out);
MH_API mh_status mh_plan_destroy(mh_plan* plan);
MH_API mh_status mh_plan_get_info(const mh_plan* plan, mh_plan_info* info);
MH_API mh_status mh_plan_set_cost(mh_plan* plan, const uint8_t* bytes, int32_t mem);
MH_API mh_status mh_plan_set_cost_from_nav(mh_plan* plan, const mh_nav* nav);
MH_API mh_status mh_plan_field(mh_plan* plan, const int32_t* goals_xy, size_t n_goals, uint32_t passable_below, const uint16_t* price,
                               size_t n_price);
MH_API mh_status mh_plan_trace(const mh_plan* plan, const int32_t* starts_xy, size_t n_starts, uint32_t cap, int32_t* out_xy,
                               uint32_t* out_len);
MH_API mh_status mh_plan_download(const mh_plan* plan, uint32_t* field);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_PLAN_H_ */
