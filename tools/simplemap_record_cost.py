"""What recording key-frames costs the odometry: the default pipeline over a synthetic drive with params.simplemap.generate off
and on (the reference's spacing formulas), the two alternating, host clock around the scans after the first six (onLidar
blocks until the scan is registered).  Usage: python tools/simplemap_record_cost.py [n_scans]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from mola_lidar_odometry_amd import synth
from mola_lidar_odometry_amd import _mp2p_icp_hip as H

PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
drive = synth.make_drive(n)
WARM = 6


def run(generate):
    os.environ["MOLA_GENERATE_SIMPLEMAP"] = "true" if generate else "false"
    os.environ["MOLA_SIMPLEMAP_OUTPUT"] = ""   # (nothing is written at the end)
    lo = H.LidarOdometry()
    lo.initialize(H.Config.FromYamlFile(PIPE))
    t0 = None
    for k, ((xyz, t), st) in enumerate(zip(drive["scans"], drive["stamps"])):
        if k == WARM:
            t0 = time.perf_counter()
        lo.onLidar(st, xyz, t)
    dt = time.perf_counter() - t0
    kf = lo.keyFrames()
    with_points = sum(f["layers"] is not None for f in kf["frames"])
    pts = sum(len(l[1]) for f in kf["frames"] if f["layers"] is not None for l in f["layers"])
    store = lo.profile().get("onLidar.5.store_keyframe", 0.0)
    return (n - WARM) / dt, with_points, pts, store


rates = {False: [], True: []}
for rep in range(6):
    for g in (False, True):
        r, k, pts, store = run(g)
        if rep:
            rates[g].append(r)
        if g:
            last = (k, pts, store)
off, on = float(np.median(rates[False])), float(np.median(rates[True]))
print("generate off: %.1f scans/s   on: %.1f scans/s (median of 5 after a warm-up run, %d scans each); %d key-frames with %d points in all, "
      "%.3f ms of host time per key-frame in store_keyframe" % (off, on, n - WARM, last[0], last[1], 1e3 * last[2] / max(last[0], 1)))
print(json.dumps({"simplemap_record_cost": dict(scans_per_s_off=off, scans_per_s_on=on, off_all=rates[False], on_all=rates[True], keyframes=last[0],
                                                keyframe_points=last[1], store_ms_per_keyframe=1e3 * last[2] / max(last[0], 1))}))
