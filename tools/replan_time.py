"""Times of include/molahip_replan.h on the 4096 x 4096 random planes of profiles/route_planning.md (a goal in the corner, prices
1 + c // 16): a block of 32 x 32 lethal cells is set and then cleared at three places -- far from the goal, midway, and next to it --
by mh_replan_update_cost as it is (withdraw, then relax from the touched tiles) and with MH_REPLAN_FULL=1 (the bytes patched, the
whole field computed from nothing), the two alternating on the same handle: set and clear bring the handle back to the state it had,
so every repeat starts from the same field.  What an update replaces, mh_plan_set_cost of the whole window + mh_plan_field, is timed
in the same run on the same planes.

  python tools/replan_time.py [OUT.json]   host clock around calls that end in a device synchronise, one warm-up round, then the
                                           median of the repeats; prints one JSON line per row and, with OUT.json, writes the rows

In the warm-up round the field after each repaired update is downloaded and compared with the one MH_REPLAN_FULL=1 leaves: the same
bits."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from mola_lidar_odometry_amd import capi, capi_nav as cn, capi_plan as cp, capi_replan as cr

WARM, REPS = 1, 5
NX = NY = 4096
SHARES = [1e-3, 1e-5]
BLOCK = 32
PLACES = [("far", 3900, 3900), ("midway", 2048, 2048), ("next_to_goal", 2, 2)]

ctx = capi.Context(0)
rows = []
ms = lambda t: round(1e3 * float(np.median(t)), 3)
med = lambda v: int(np.median(v))
price = (1 + np.arange(253) // 16).astype(np.uint16)
goal = np.array([[0, 0]], np.int32)
lethal = np.full((BLOCK, BLOCK), cn.LETHAL, np.uint8)


def clocked(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


for share in SHARES:
    rng = np.random.default_rng(int(share * 1e6))
    cost = rng.integers(0, 253, (NY, NX)).astype(np.uint8)
    cost.reshape(-1)[rng.choice(NX * NY, int(NX * NY * share), replace=False)] = cn.LETHAL
    cost[0, 0] = 0
    plan = cp.PlanMap(ctx, NX, NY).set_cost(cost).field(goal, price)
    # what an update replaces: the whole window set again and the field from nothing
    whole = [clocked(lambda: plan.set_cost(cost).field(goal, price)) for _ in range(WARM + REPS)][WARM:]
    field_only = [clocked(lambda: plan.field(goal, price)) for _ in range(WARM + REPS)][WARM:]
    i = plan.info()
    rows.append(dict(window=[NX, NY], lethal_share=share, set_cost_and_field_ms=ms(whole), field_ms=ms(field_only), sweeps=int(i.n_sweeps),
                     tile_runs=int(i.n_tile_runs), reached=int(i.n_reached)))
    print(json.dumps(rows[-1]), flush=True)
    for name, x0, y0 in PLACES:
        old = cost[y0:y0 + BLOCK, x0:x0 + BLOCK].copy()
        seen = {}
        for rep in range(WARM + REPS):
            for mode in (("repair", "full") if rep % 2 == 0 else ("full", "repair")):        # the two alternate
                if mode == "full":
                    os.environ["MH_REPLAN_FULL"] = "1"
                for step, new in (("set", lethal), ("clear", old)):
                    dt = clocked(lambda: cr.update_cost(plan, x0, y0, new))
                    ri = cr.info(plan)
                    if rep >= WARM:
                        seen.setdefault((step, mode), []).append((dt, ri.n_withdraw_sweeps, ri.n_relax_sweeps, int(ri.n_tile_runs_withdraw),
                                                                  int(ri.n_tile_runs_relax), int(ri.n_withdrawn), int(ri.n_cells_repriced)))
                    else:
                        f = plan.download()
                        if (step, "bits") in seen:
                            assert np.array_equal(seen[(step, "bits")], f), (name, step)      # the same bits either way
                            del seen[(step, "bits")]
                        else:
                            seen[(step, "bits")] = f
                        del f
                os.environ.pop("MH_REPLAN_FULL", None)
        for step in ("set", "clear"):
            row = dict(window=[NX, NY], lethal_share=share, place=name, block=[x0, y0, BLOCK, BLOCK], step=step)
            for mode in ("repair", "full"):
                v = np.array(seen[(step, mode)], np.float64)
                row.update({mode + "_ms": ms(v[:, 0]), mode + "_ms_min": round(1e3 * float(v[:, 0].min()), 3), mode + "_ms_max": round(1e3 * float(v[:, 0].max()), 3),
                            mode + "_withdraw_sweeps": med(v[:, 1]), mode + "_relax_sweeps": med(v[:, 2]), mode + "_tile_runs_withdraw": med(v[:, 3]),
                            mode + "_tile_runs_relax": med(v[:, 4])})
            row.update(withdrawn=med(np.array(seen[(step, "repair")])[:, 5]), cells_repriced=med(np.array(seen[(step, "repair")])[:, 6]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    plan.close()
if len(sys.argv) > 1:
    json.dump(dict(rows=rows), open(sys.argv[1], "w"))
