"""Times of include/molahip_nav.h: mh_nav_inflate (the column pass and the row pass) and mh_nav_reach (the sweeps) on windows of
4096 x 4096 cells and of one row of 2^26 cells, at R = 8, 30 and 255, with the row pass's early stop and without it
(MH_NAV_NO_EARLY_STOP, read per call), and the whole build_costmap_from_keyframes on the outdoor scenario of tests/elev_cases.py.

Two modes.
  python tools/nav_time.py [OUT.json]          runs the calls: host clock around calls that end in a device synchronise, one
                                               warm-up, then the median of the repeats; prints one JSON line and, with OUT.json,
                                               writes the order of the calls for the second mode
  python tools/nav_time.py --trace OUT.json KERNEL_TRACE.csv
                                               reads the kernel trace that `rocprofv3 --kernel-trace --output-format csv` wrote over
                                               a run of the first mode and gives every call its kernels' times: the dispatches of
                                               k_nav_* are taken in order of their start and handed to the calls in the order of
                                               OUT.json (an inflate call is one k_nav_col and one k_nav_row; a reach call is one
                                               k_nav_seed, its sweeps of k_nav_reach and one k_nav_count)
The base planes are random: a share of lethal cells (1e-3: an obstacle every 32 cells or so each way; 1e-5: open ground, where the
column pass walks far), costs of 0 under the rest."""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

WARM, REPS = 1, 5
WINDOWS = [(4096, 4096), (1 << 26, 1)]
RADII = [8, 30, 255]
SHARES = [1e-3, 1e-5]


def trace_mode(plan_path, csv_path):
    plan = json.load(open(plan_path))["calls"]
    rows = [r for r in csv.DictReader(open(csv_path)) if "k_nav_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    kern = [(("col" if "k_nav_col" in r["Kernel_Name"] else "row" if "k_nav_row" in r["Kernel_Name"] else "seed" if "k_nav_seed" in r["Kernel_Name"]
              else "reach" if "k_nav_reach" in r["Kernel_Name"] else "count"), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    at, out = 0, {}
    for call in plan:
        label, kind = call["label"], call["kind"]
        if kind == "inflate":
            assert kern[at][0] == "col" and kern[at + 1][0] == "row", (label, kern[at:at + 2])
            out.setdefault(label, dict(col_us=[], row_us=[]))
            out[label]["col_us"].append(kern[at][1])
            out[label]["row_us"].append(kern[at + 1][1])
            at += 2
        else:
            assert kern[at][0] == "seed", (label, kern[at])
            at += 1
            sweeps = []
            while at < len(kern) and kern[at][0] == "reach":
                sweeps.append(kern[at][1])
                at += 1
            if at < len(kern) and kern[at][0] == "count":
                at += 1
            d = out.setdefault(label, dict(sweeps=[], sweep_us=[], sweep_us_max=[]))
            d["sweeps"].append(len(sweeps))
            d["sweep_us"].append(float(np.median(sweeps)) if sweeps else 0.0)
            d["sweep_us_max"].append(max(sweeps) if sweeps else 0.0)
    for label, d in out.items():
        print(json.dumps(dict(label=label, **{k: (round(float(np.median(v[WARM:] or v)), 1) if k != "sweeps" else v[-1]) for k, v in d.items()})))
    print(json.dumps(dict(dispatches=len(kern), handed_out=at)))


if len(sys.argv) > 1 and sys.argv[1] == "--trace":
    trace_mode(sys.argv[2], sys.argv[3])
    sys.exit(0)

from mola_lidar_odometry_amd import capi, capi_nav as cn

ctx = capi.Context(0)
calls, rows = [], []
ms = lambda t: round(1e3 * float(np.median(t)), 3)


def timed(fn, label, kind):
    ts = []
    for rep in range(WARM + REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        calls.append(dict(label=label, kind=kind))
        if rep >= WARM:
            ts.append(dt)
    return ts


for nx, ny in WINDOWS:
    for share in SHARES:
        rng = np.random.default_rng(nx % 1000 + int(share * 1e6))
        base = np.zeros((ny, nx), np.uint8)
        base.reshape(-1)[rng.choice(nx * ny, int(nx * ny * share), replace=False)] = cn.LETHAL
        at = int(np.argmax(base.reshape(-1) == 0))                                 # the first free cell
        seed = np.array([[at % nx, at // nx]], np.int32)
        nav = cn.NavMap(ctx, nx, ny).set_base(base)
        for Rc in RADII:
            table = np.minimum(253, 253 * 4 // (np.arange(Rc * Rc + 1) + 4)).astype(np.uint8)      # 253 up to d2 = 0, falling: cells near obstacles are impassable
            table[1:min(len(table), 5)] = 253
            row = dict(window=[nx, ny], lethal_share=share, R=Rc)
            for name, env in (("early_stop", None), ("no_early_stop", "1")):
                if env:
                    os.environ["MH_NAV_NO_EARLY_STOP"] = env
                label = "%dx%d share %g R %d %s" % (nx, ny, share, Rc, name)
                row["inflate_ms_" + name] = ms(timed(lambda: nav.inflate(Rc, table), label, "inflate"))
                os.environ.pop("MH_NAV_NO_EARLY_STOP", None)
                planes = nav.download(reach=False)
                if name == "early_stop":
                    first = planes
                else:
                    assert np.array_equal(first[0], planes[0]) and np.array_equal(first[1], planes[1])       # the same bits either way
                del planes
            label = "%dx%d share %g R %d reach" % (nx, ny, share, Rc)
            row["reach_ms"] = ms(timed(lambda: nav.reach(seed, 253), label, "reach"))
            i = nav.info()
            row.update(sweeps=int(i.n_sweeps), reached=int(i.n_reached), passable=int((first[1] < 253).sum()))
            del first
            rows.append(row)
            print(json.dumps(row), flush=True)
        nav.close()

# the whole host path on the outdoor scenario (12 key-frames, 642 017 points, a window of 404 x 54 cells)
import elev_cases as ec
import nav_cases as nc
from mola_lidar_odometry_amd import _mp2p_icp_hip as H

_, kfset = ec.scenario()
for inscribed, inflation, unknown in ((1.0, 2.0, False), (2.0, 3.0, True), (2.0, 3.0, False)):
    text = nc.scenario_pipeline(inscribed, inflation, unknown, "first")
    best = None
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        c = H.build_costmap_from_keyframes(kfset, text)
        dt = time.perf_counter() - t0
        calls.append(dict(label="scenario %g %g %s" % (inscribed, inflation, unknown), kind="inflate"))
        calls.append(dict(label="scenario %g %g %s reach" % (inscribed, inflation, unknown), kind="reach"))
        if rep >= WARM and (best is None or dt < best[0]):
            best = (dt, c)
    dt, c = best
    row = dict(scenario=[inscribed, inflation, unknown], build_costmap_from_keyframes_ms=round(1e3 * dt, 3), source_ms=round(1e3 * c["seconds_source"], 3),
               inflate_ms=round(1e3 * c["seconds_inflate"], 3), reach_ms=round(1e3 * c["seconds_reach"], 3), sweeps=c["sweeps"],
               reached=c["cells_reached"], keyframes_blocked=c["keyframes_blocked"])
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    json.dump(dict(calls=calls, rows=rows), open(sys.argv[1], "w"))
