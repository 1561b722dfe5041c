"""Cost of allowMatchAlreadyMatchedGlobalPoints: false (unique_global, U13) on the multi-layer device loop: the creal workload
(its decimated scan against the 1 M-point map) as ONE pair through mh_icp_align_layers / mh_icp_align_layers_opts, the stall test
off so that both routes run all --iters ICP iterations.  Median of --reps warmed alignments, host clock around the calls;
microseconds per ICP iteration = that / iterations.

    python tools/unique_global_bench.py [--reps 200] [--iters 40] [--mode both|plain|unique]

Kernel durations: rocprofv3 --kernel-trace --stats -- python tools/unique_global_bench.py --mode unique --reps 20
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mola_lidar_odometry_amd import capi, synth  # noqa: E402


def _sched(v, n):
    """n values of a schedule: the workload's own, its last value repeated beyond its end."""
    v = np.atleast_1d(np.asarray(v, np.float64))
    return np.ascontiguousarray(np.concatenate([v, np.full(max(0, n - len(v)), v[-1])])[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--mode", default="both", choices=("both", "plain", "unique"))
    a = ap.parse_args()
    w = synth.workload_creal()
    ctx = capi.Context(0)
    m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
    s = capi.Scan(ctx, w.scan_xyz)
    thr, kp = _sched(w.threshold, a.iters), _sched(w.kernel_param, a.iters)
    p = capi.ICPParams(max_iterations=a.iters, threshold=1.0, kernel_param=kp, disable_stall_test=True)
    print("scan points %d, map points %d, %d iterations" % (len(w.scan_xyz), len(w.map_xyz), a.iters))
    for name, flag in (("plain", 0), ("unique", 1)):
        if a.mode not in ("both", name):
            continue
        pairs = [dict(map=m, scan=s, threshold=thr, unique_global=flag)]
        for _ in range(10):
            capi.icp_align_layers(pairs, w.T_guess, p, want_trace=False)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = capi.icp_align_layers(pairs, w.T_guess, p, want_trace=False)
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        print("%-6s %.3f ms / alignment, %.2f us / ICP iteration  (%d iterations, %s, %d of %d paired, %d host polls)" % (
            name, ms, 1e3 * ms / max(1, r["n_iterations"]), r["n_iterations"], capi.TERM_NAMES[r["termination_reason"]],
            r["n_final_pairs"], r["potential_pairings"], r["n_host_polls"]))


if __name__ == "__main__":
    main()
