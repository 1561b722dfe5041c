"""Stage times of mola_hip::clean_keyframes on the two scenarios of profiles/map_cleaning.md: the 20-frame street with its mover
(tests/clean_cases.py) and the 66-frame loop scenario (tests/loop_cases.py).  One warm-up call, then N timed calls through the
Python module; per stage the median and the range of CleaningReport::seconds, and the whole call by the host clock.
    python tools/clean_time.py [--calls 20] [--once street|loop]     (--once: one warm-up and one call, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scenarios(which):
    import clean_cases as cc
    import loop_cases as lc
    out = {}
    if which in (None, "street"):
        s = cc.scenario()
        out["street"] = cc.keyframe_set(s["poses"], s["sweeps"])
    if which in (None, "loop"):
        s = lc.scenario()
        out["loop"] = lc.keyframe_set(s["est"], s["sweeps"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    from mola_lidar_odometry_amd import _mp2p_icp_hip as host
    for name, kf in scenarios(a.once).items():
        host.clean_keyframes(kf, None)  # warm-up: code objects, first allocations
        stages, whole, rep = {"views": [], "votes": [], "removal": []}, [], None
        for _ in range(1 if a.once else a.calls):
            t0 = time.perf_counter()
            _, rep = host.clean_keyframes(kf, None)
            whole.append(time.perf_counter() - t0)
            for k in stages:
                stages[k].append(rep["seconds"][k])
        row = dict(scenario=name, frames=len(kf["frames"]), points_in=rep["points_in"], points_removed=rep["points_removed"], pairs=rep["pairs"],
                   calls=len(whole), whole_ms=[round(1e3 * f(whole), 3) for f in (np.median, np.min, np.max)])
        for k, v in stages.items():
            row[k + "_ms"] = [round(1e3 * f(v), 3) for f in (np.median, np.min, np.max)]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
