/* molahip_replan.h -- repairing the cost-to-go field of an mh_plan after the cost of a rectangle of cells changed: the ninth public
 * header of libmolahip.so.  It adds to include/molahip_plan.h and changes nothing there: MH_PLAN_API_VERSION,
 * mh_plan_info and MH_ABI_VERSION stay what they are, this surface has a version of its own.  Conventions (status codes, `mem`
 * spaces, streams, ownership) are molahip.h's; the planes, the field rule and the trace rule are molahip_plan.h's.
 *
 * mh_replan_update_cost(plan, x0, y0, w, h, bytes, mem) -- `bytes` is an array of h * w uint8, y outer (entry [r * w + c] is the new
 *   cost of the cell in column x0 + c of row y0 + r), in the memory space `mem` (MH_MEM_HOST, MH_MEM_DEVICE or MH_MEM_HOST_PINNED).
 *   It replaces the cost of the cells [x0, x0 + w) x [y0, y0 + h).  The call is synchronous: on return the caller's array may be
 *   reused.
 *
 * mh_replan_update_cost_from_nav(plan, nav, x0, y0, w, h) -- the same, the rectangle taken out of the cost plane of an mh_nav, device
 *   to device.  MH_ERR_INVALID_ARGUMENT, the handle untouched, on mh_plan_set_cost_from_nav's three conditions: `nav` has no valid
 *   cost, its nx or ny differ from the plan's, or it was created on another context.
 *
 *   THE UPDATE RULE.
 *   NO VALID FIELD (has_field == 0).  The bytes are replaced and nothing else happens: a later mh_plan_field sees the patched plane.
 *   n_cells_changed is counted; there are no prices to compare, so n_cells_repriced is 0, as is every other figure.
 *   A VALID FIELD.  On return the plan is, bit for bit, what mh_plan_set_cost(the new plane) followed by mh_plan_field(the same goals,
 *   the same passable_below, the same prices) would have left: the field plane -- and with it what mh_plan_trace and mh_plan_download
 *   give -- and mh_plan_info's n_reached, max_field, n_goals_blocked, n_goals_outside, passable_below and has_field.  n_sweeps and
 *   n_tile_runs of mh_plan_info become those of the update's relax phase (n_relax_sweeps, n_tile_runs_relax below).  The plan keeps the
 *   goals and the price table of its last mh_plan_field on the device for this.  A goal whose cell closes stops being a goal and counts
 *   as blocked; a blocked goal whose cell opens becomes one.
 *   REPRICED.  A cell of the rectangle is changed when its byte differs, and repriced when its passability or its price differs (two
 *   bytes at or above passable_below are both impassable; two passable bytes may share a price).
 *   WITHDRAWN.  Let F be the field before the call, and take the new plane.  A set S of cells is self-supporting when every c in S is
 *   passable, has F[c] finite, and either has F[c] == 0 or has a neighbour n in S, by a step the field rule allows on the new plane,
 *   with F[n] + w(c, n) <= F[c].  The union of self-supporting sets is self-supporting; K is the largest one.  n_withdrawn = the cells
 *   with F finite that are not in K: the values that rested, directly or through others, on something the update took away.  Every
 *   step weight is at least 10, so support strictly descends and cannot go round in a circle; K does not depend on the order in which
 *   cells are taken out, so the count is exact and the same from run to run.  The values of K are lengths of real paths on the new
 *   plane, hence upper bounds of the new field, and relaxing from them gives it.
 *   TWO CONSEQUENCES.  An update that only lowers prices or opens cells has n_withdrawn == 0.  An update with n_cells_repriced == 0
 *   launches no sweep of either kind: n_withdraw_sweeps, n_relax_sweeps and both tile counts are 0, and so are mh_plan_info's n_sweeps
 *   and n_tile_runs.
 *   (Shape: a lane per rectangle cell writes the byte, takes the field of a cell that closed back to MH_PLAN_UNREACHED and flags the
 *   tiles round a repriced cell.  Withdraw sweeps over the flagged tiles follow, the tile and its image those of mh_plan_field: rounds
 *   in LDS take back every finite value above 0 that no neighbour supports until none is left, the HOST repeats sweeps until one changes
 *   nothing; n_withdraw_sweeps = the sweeps launched, n_tile_runs_withdraw = the tiles that staged, summed over them.  The goals are
 *   placed again, and mh_plan_field's relax sweeps run from the tiles the patch or a withdrawal touched.  The sweep and tile counts may
 *   differ from run to run; the planes and every other figure do not.  No workgroup waits for another.  With MH_PLAN_ALL_TILES=1 every
 *   tile runs in every sweep of both kinds.  With MH_REPLAN_FULL=1 in the environment, read per call, an update with a repriced cell
 *   patches the bytes and computes the whole field from nothing -- n_withdrawn and the withdraw figures are then 0: for measuring, and
 *   as a twin in tests; the same planes.)
 *   With no goal inside the window the field is all MH_PLAN_UNREACHED before and after, and no sweep is launched.
 *   MH_ERR_INTERNAL when the sweeps do not come to rest within nx * ny of them (they always do); the field is then invalid.
 *
 * mh_replan_get_info -- the figures of the last update since the last mh_plan_set_cost or mh_plan_field (all 0 when there was none;
 *   n_updates counts the updates since the last mh_plan_field).
 *
 * Refusals.  MH_ERR_INVALID_ARGUMENT before any device work, the handle untouched: a NULL argument; a bad `mem`; w or h of 0; x0 + w >
 *   nx or y0 + h > ny, computed in 64 bits; no cost plane (mh_plan_set_cost comes first); the three conditions on `nav`.
 *
 * NOT BUILT: a change of goals or prices (that is mh_plan_field); a moving window; several rectangles per call; any-angle or
 * kinematic routes.
 *
 * Threads.  As molahip_plan.h: an mh_plan is not to be used by two calls at once. */
#ifndef MOLAHIP_REPLAN_H_
#define MOLAHIP_REPLAN_H_

#include "molahip_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_REPLAN_API_VERSION 1

typedef struct {
  uint64_t n_cells_changed;      /* offset 0: cells of the rectangle whose byte differs */
  uint64_t n_cells_repriced;     /* 8: those whose passability or price differs */
  uint64_t n_withdrawn;          /* 16: cells with a finite field outside the largest self-supporting set */
  uint64_t n_tile_runs_withdraw; /* 24: tiles that staged in a withdraw sweep, over all of them */
  uint64_t n_tile_runs_relax;    /* 32: tiles that staged and relaxed, over all relax sweeps */
  uint32_t n_withdraw_sweeps;    /* 40: withdraw sweeps launched, the last of which changed nothing */
  uint32_t n_relax_sweeps;       /* 44: relax sweeps launched, the last of which changed nothing */
  uint64_t n_updates;            /* 48: updates since the last mh_plan_field */
  uint64_t reserved_;            /* 56 */
} mh_replan_info;                /* 64 bytes */

/* MH_REPLAN_API_VERSION of the loaded library. */
MH_API uint32_t mh_replan_api_version(void);
MH_API mh_status mh_replan_update_cost(mh_plan* plan, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint8_t* bytes, int32_t mem);
MH_API mh_status mh_replan_update_cost_from_nav(mh_plan* plan, const mh_nav* nav, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
MH_API mh_status mh_replan_get_info(const mh_plan* plan, mh_replan_info* info);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_REPLAN_H_ */
