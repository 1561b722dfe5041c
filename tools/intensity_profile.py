"""Numbers of profiles/intensity_c2.txt.  `kernels`: mh_scan_normalize_intensity and mh_scan_by_intensity on the C2 scan,
--calls times each (run it under rocprofv3 --kernel-trace --stats).  `driver`: the stand-alone driver on synth.make_drive(14)
with synth.drive_intensities, the intensity chain of tests/test_odometry_intensity.py against the default chain -- scans/s
(host wall time of onLidar, mean of --runs timed runs after one warm-up run) and the intensity chain's ATE.

    python tools/intensity_profile.py kernels [--calls 50]
    python tools/intensity_profile.py driver [--runs 2]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(calls):
    from mola_lidar_odometry_amd import capi, synth
    xyz = np.asarray(synth.workload_c2().scan_xyz, np.float32)
    p = xyz.astype(np.float64)
    inten = (40.0 + 30.0 * np.sin(0.7 * p[:, 0]) * np.cos(0.3 * p[:, 1]) + 5.0 * p[:, 2]).astype(np.float32)
    ctx = capi.Context(0)
    s = capi.Scan(ctx, xyz).set_intensity(inten)
    outs = [capi.Scan(ctx) for _ in range(3)]
    rng = np.array([np.nan, np.nan], np.float32)
    for _ in range(calls):
        s.set_intensity(inten)  # (the same input every call: normalising a normalised layer would be another workload)
        s.normalize_intensity(rng)
    for _ in range(calls):
        s.by_intensity(capi.by_intensity_params(0.1, 0.9), *outs)
    print(f"C2 scan: {len(xyz)} points; by-intensity outputs low {len(outs[0])} mid {len(outs[1])} high {len(outs[2])}")


def driver(runs):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H, synth
    spec = importlib.util.spec_from_file_location("_t", os.path.join(ROOT, "tests", "test_odometry_intensity.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    d = synth.make_drive(14)
    d["intensity"] = synth.drive_intensities(d)
    for name, text in (("default chain", open(t.chains.PIPE).read()), ("intensity chain", t.pipeline())):
        rates = []
        for r in range(runs + 1):
            lo = H.LidarOdometry(0, True)
            lo.setIntensityInput(True)
            lo.initialize(H.Config.FromYamlText(text))
            recs = [t._records(d, k) for k in range(len(d["scans"]))]
            t0 = time.perf_counter()
            for k, rec in enumerate(recs):
                lo.onLidar(float(d["stamps"][k]), rec, None, [0, 1, 2], 3, 4)
            dt = time.perf_counter() - t0
            if r:
                rates.append(len(recs) / dt)
        ate = t.chains._ate(lo.records(), d)
        print(f"{name}: {np.mean(rates):.0f} scans/s (runs {', '.join(f'{v:.0f}' for v in rates)}), ATE RMSE {ate:.4f} m")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "driver"])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    kernels(a.calls) if a.what == "kernels" else driver(a.runs)
