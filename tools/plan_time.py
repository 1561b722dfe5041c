"""Times of include/molahip_plan.h: mh_plan_field on windows of 4096 x 4096 cells with a goal in the corner -- with the active-tile
flags and with every tile in every sweep (MH_PLAN_ALL_TILES, read per call) --, mh_nav_reach on the same plane beside it,
mh_plan_trace for 1 and for 1000 starts, and the whole plan_route_from_keyframes on the outdoor scenario of tests/elev_cases.py.

  python tools/plan_time.py [OUT.json]     host clock around calls that end in a device synchronise, one warm-up, then the median of
                                           the repeats; prints one JSON line per row and, with OUT.json, writes the rows

The cost planes are random: a share of lethal cells (1e-3: an obstacle every 32 cells or so each way; 1e-5: open ground), costs of
0 .. 252 under the rest, priced 1 + c // 16."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from mola_lidar_odometry_amd import capi, capi_nav as cn, capi_plan as cp

WARM, REPS = 1, 5
NX = NY = 4096
SHARES = [1e-3, 1e-5]

ctx = capi.Context(0)
rows = []
ms = lambda t: round(1e3 * float(np.median(t)), 3)


def timed(fn):
    ts = []
    for rep in range(WARM + REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if rep >= WARM:
            ts.append(dt)
    return ts


price = (1 + np.arange(253) // 16).astype(np.uint16)
for share in SHARES:
    rng = np.random.default_rng(int(share * 1e6))
    cost = rng.integers(0, 253, (NY, NX)).astype(np.uint8)
    cost.reshape(-1)[rng.choice(NX * NY, int(NX * NY * share), replace=False)] = cn.LETHAL
    cost[0, 0] = 0
    goal = np.array([[0, 0]], np.int32)
    plan = cp.PlanMap(ctx, NX, NY).set_cost(cost)
    row = dict(window=[NX, NY], lethal_share=share)
    first = None
    for name, env in (("active_tiles", None), ("all_tiles", "1")):
        if env:
            os.environ["MH_PLAN_ALL_TILES"] = env
        sweeps, runs = [], []

        def call():
            plan.field(goal, price)
            i = plan.info()
            sweeps.append(int(i.n_sweeps))
            runs.append(int(i.n_tile_runs))

        row["field_ms_" + name] = ms(timed(call))
        os.environ.pop("MH_PLAN_ALL_TILES", None)
        row["sweeps_" + name] = int(np.median(sweeps[WARM:]))
        row["tile_runs_" + name] = int(np.median(runs[WARM:]))
        f = plan.download()
        if first is None:
            first = f
        else:
            assert np.array_equal(first, f)                                        # the same bits either way
        del f
    i = plan.info()
    row.update(reached=int(i.n_reached), max_field=int(i.max_field), tiles=(NX // cp.TILE_X) * (NY // cp.TILE_Y))
    # the routes: 1 start in the far corner region, 1000 random ones
    finite = np.argwhere(first != cp.UNREACHED)[:, ::-1].astype(np.int32)
    far = finite[-1:]
    many = finite[rng.integers(0, len(finite), 1000)]
    cap = 16384
    lens = {}
    for starts in (far, many):                                                     # (the C call alone: the output arrays are made once)
        n = len(starts)
        starts = np.ascontiguousarray(starts, np.int32)
        out = np.zeros((n, cap, 2), np.int32)
        lens[n] = np.zeros(n, np.uint32)
        call = lambda: cp._chk(cp.lib().mh_plan_trace(plan._h, starts.ctypes.data_as(cp._I32P), n, cap, out.ctypes.data_as(cp._I32P),
                                                      lens[n].ctypes.data_as(cp._U32P)))
        row["trace_ms_1_start" if n == 1 else "trace_ms_1000_starts"] = ms(timed(call))
        del out
    row.update(route_cells_1_start=int(lens[1][0]), route_cells_1000_starts_median=int(np.median(lens[1000])), route_cells_1000_starts_max=int(lens[1000].max()))
    del first, finite
    plan.close()
    # mh_nav_reach over the same passable cells: the only earlier figure of the same shape
    nav = cn.NavMap(ctx, NX, NY).set_base(cost).inflate(0, np.zeros(1, np.uint8))
    row["nav_reach_ms"] = ms(timed(lambda: nav.reach(goal, 253)))
    row.update(nav_reach_sweeps=int(nav.info().n_sweeps), nav_reached=int(nav.info().n_reached))
    nav.close()
    rows.append(row)
    print(json.dumps(row), flush=True)

# the whole host path on the outdoor scenario (12 key-frames, a window of 404 x 54 cells): the costmap, then the route
import elev_cases as ec
import plan_cases as pc
from mola_lidar_odometry_amd import _mp2p_icp_hip as H

_, kfset = ec.scenario()
for inscribed, inflation, unknown in ((1.0, 2.0, False), (2.0, 3.0, True), (2.0, 3.0, False)):
    text = pc.scenario_pipeline(inscribed, inflation, unknown)
    ts, r = [], None
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        r = H.plan_route_from_keyframes(kfset, text)
        if rep >= WARM:
            ts.append(time.perf_counter() - t0)
    c = r["costmap"]
    row = dict(scenario=[inscribed, inflation, unknown], plan_route_from_keyframes_ms=ms(ts), status=r["status"], cells=len(r["cells"]),
               length_m=round(r["length_m"], 3), cost_to_go=r["cost_to_go"], field_ms=round(1e3 * r["seconds_field"], 3),
               trace_ms=round(1e3 * r["seconds_trace"], 3), sweeps=r["sweeps"], tile_runs=r["tile_runs"],
               costmap_ms=round(1e3 * (c["seconds_source"] + c["seconds_inflate"] + c["seconds_reach"]), 3))
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    json.dump(dict(rows=rows), open(sys.argv[1], "w"))
