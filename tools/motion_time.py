"""Times mh_scan_deskew_motion / mh_scan_deskew_motion_pair (include/molahip_motion.h) against mh_scan_deskew / mh_scan_deskew_pair
on one device, on a 64 x 1875 sweep of the benchmark's street scene (about 120 k points, stamps by azimuth) with a 4 096-point
small layer for the pairs, at K = 12 and K = 64.

Single calls are queued (nothing is read back): `--calls` of them back to back, one synchronise, host clock around both -- the time
per call of a saturated stream, launch cost included.  Pair calls wait for their box, so each is timed on its own and the figure is
the median.  The variants alternate inside every round; the table gives the median over the rounds and their spread.  With
--once every variant runs a few times only: the run to put under a kernel trace (kernel times come from there, not from here).

    python tools/motion_time.py [--rounds 7] [--calls 200] [--once] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mola_lidar_odometry_amd import capi, capi_motion as cm, synth, trajectory  # noqa: E402


def so3_exp(w):
    return synth._so3_exp(np.asarray(w, np.float64).reshape(1, 3))[0]


def table(K, w, v):
    knots = -0.06 + 0.12 / K * np.arange(K)
    R = np.stack([so3_exp(w * k) for k in knots])
    return cm.motion_table(knots, R, np.tile(w, (K, 1)), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if capi.device_count() == 0:
        raise SystemExit("motion_time.py: no device")
    scene = synth.make_scene()
    xyz = synth.make_scan(scene, [0.0, 0.0, synth.SENSOR_H, 0.0, 0.0, 0.0], 64, 1875)
    t = trajectory.kitti_azimuth_timestamps(xyz, 0.1).astype(np.float32)
    order = np.argsort(t, kind="stable")  # raw order is time order
    xyz, t = xyz[order], t[order]
    small_idx = np.linspace(0, len(xyz) - 1, 4096).astype(int)
    ctx = capi.Context(0)
    big = capi.Scan(ctx, xyz).set_timestamps(t)
    small = capi.Scan(ctx, xyz[small_idx]).set_timestamps(t[small_idx])
    out, out_s = capi.Scan(ctx), capi.Scan(ctx)
    v, w = np.array([12.0, 0.3, 0.0]), np.array([0.02, -0.03, 0.4])
    tw = np.concatenate([v, w])
    keep12, T12 = table(12, w, v)
    keep64, T64 = table(64, w, v)
    singles = {"mh_scan_deskew": lambda: big.deskew(tw, out), "mh_scan_deskew_motion K=12": lambda: cm.deskew_motion(big, T12, out),
               "mh_scan_deskew_motion K=64": lambda: cm.deskew_motion(big, T64, out)}
    pairs = {"mh_scan_deskew_pair": lambda: big.deskew_pair(small, tw, out, out_s),
             "mh_scan_deskew_motion_pair K=12": lambda: cm.deskew_motion_pair(big, small, T12, out, out_s),
             "mh_scan_deskew_motion_pair K=64": lambda: cm.deskew_motion_pair(big, small, T64, out, out_s)}
    n_warm = 3 if a.once else 30
    for f in list(singles.values()) + list(pairs.values()):
        for _ in range(n_warm):
            f()
    ctx.synchronize()
    ref = out.download()["xyz"].copy()
    for name, f in singles.items():  # the three agree on a constant rate (within a float ulp): the same work is being timed
        f()
        d = np.abs(out.download()["xyz"].astype(np.float64) - ref)
        assert (d <= np.spacing(np.maximum(np.abs(ref), 1e-3).astype(np.float32))).all(), name
    if a.once:
        print(json.dumps({"points": int(len(xyz)), "once": True}))
        return
    res = {k: [] for k in list(singles) + list(pairs)}
    for _ in range(a.rounds):
        for name, f in singles.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            ctx.synchronize()
            res[name].append((time.perf_counter() - t0) / a.calls)
        for name, f in pairs.items():
            each = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                f()
                each.append(time.perf_counter() - t0)
            res[name].append(float(np.median(each)))
    table_out = {k: dict(median_us=1e6 * float(np.median(x)), min_us=1e6 * float(np.min(x)), max_us=1e6 * float(np.max(x))) for k, x in res.items()}
    result = dict(points=int(len(xyz)), small_points=4096, rounds=a.rounds, calls=a.calls, per_call=table_out)
    print(json.dumps(result))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
