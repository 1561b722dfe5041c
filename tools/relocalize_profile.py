#!/usr/bin/env python3
"""Timings behind profiles/relocalize.md: mh_score_poses against the per-candidate alternative (one mh_nn_search per pose),
mh_map_restore against mh_map_build, and the relocalization stage of the driver.  Host clock around calls that block until
their result is on the host; every shape is warmed up; medians of repeated calls.  Prints one JSON document.

  python tools/relocalize_profile.py [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, repeat):
    fn()   # warm-up: code objects, scratch growth
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), repeat=repeat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import score_ref as sr
    from mola_lidar_odometry_amd import capi, synth
    out = {}
    ctx = capi.Context(0)

    # ---- scoring: the 13 x 13 x 9 grid of tests/score_ref.py over the 2000-point scan / 20 000-point map
    w = synth.workload_small()
    poses, _ = sr.small_grid(w)
    m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
    s = capi.Scan(ctx, w.scan_xyz)
    out["score_1521x2000"] = median_ms(lambda: capi.score_poses(m, s, poses, sr.THRESHOLD), 20)
    out["nn_search_x1521_2000"] = median_ms(lambda: [capi.nn_search(m, s, T, sr.THRESHOLD) for T in poses], 3)
    big = np.tile(poses, (44, 1))[:65536]
    out["score_65536x2000"] = median_ms(lambda: capi.score_poses(m, s, big, sr.THRESHOLD), 5)
    got = capi.score_poses(m, s, poses, sr.THRESHOLD)
    out["score_1521x2000"]["pairs_per_call"] = int(got["n_paired"].sum())
    out["score_1521x2000"]["point_pose_products"] = int(len(poses) * len(w.scan_xyz))

    # ---- the same grid over the C2 shapes: ~120 k-point scan, 1 M-point map
    c2 = synth.workload_c2()
    poses2, _ = sr.relocalization_grid(c2.pose_gt_ypr + sr.MEAN_OFFSET, sr.grid_cov(1.0, 1.0, np.deg2rad(4.0)), sr.STEP_XY, sr.STEP_YAW)
    m2 = capi.Map(ctx, c2.voxel_size, c2.cap).build(c2.map_xyz)
    s2 = capi.Scan(ctx, c2.scan_xyz)
    out["score_1521x%d" % len(c2.scan_xyz)] = median_ms(lambda: capi.score_poses(m2, s2, poses2, sr.THRESHOLD), 5)
    out["nn_search_x1_%d" % len(c2.scan_xyz)] = median_ms(lambda: capi.nn_search(m2, s2, poses2[0], sr.THRESHOLD), 10)

    # ---- snapshot: restore against build, 20 000 and 1 000 000 stored points
    for name, mm, xyz in (("20k", m, w.map_xyz), ("1M", m2, c2.map_xyz)):
        d, info = mm.download(), mm.info()
        fresh = capi.Map(ctx, float(info.voxel_size), int(info.max_points_per_voxel))
        out["download_" + name] = median_ms(lambda: mm.download(), 5)
        out["restore_" + name] = median_ms(lambda: fresh.restore(d["xyz"], d["src_idx"], info.n_offered), 5)
        out["build_" + name] = median_ms(lambda: fresh.build(xyz), 5)
        fresh.close()

    # ---- the driver's relocalization stage (the localization test's drive and request)
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    from oracle import oracle_c as oc
    pipe = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
    drive = synth.make_drive(10)
    lo = H.LidarOdometry()
    lo.initialize(H.Config.FromYamlFile(pipe))
    import tempfile
    path = os.path.join(tempfile.mkdtemp(), "session1.mhmap")
    for k in range(6):
        lo.onLidar(drive["stamps"][k], *drive["scans"][k])
    t0 = time.perf_counter()
    lo.saveLocalMaps(path)
    out["saveLocalMaps_ms"] = (time.perf_counter() - t0) * 1e3
    out["map_file_bytes"] = os.path.getsize(path)
    r6 = lo.onLidar(drive["stamps"][6], *drive["scans"][6])
    mean = np.round(oc.pose_to_ypr(np.array(r6["pose"])), 3) + np.array([0.9, -0.6, 0.0, np.deg2rad(4.0), 0.0, 0.0])
    os.environ["MOLA_LOAD_MM"] = path
    os.environ["MOLA_MAPPING_ENABLED"] = "false"
    stage = []
    for _ in range(4):
        lo2 = H.LidarOdometry()
        t0 = time.perf_counter()
        lo2.initialize(H.Config.FromYamlFile(pipe))
        t_init = (time.perf_counter() - t0) * 1e3
        lo2.relocalizeNearPose(list(synth.pose_from_ypr(mean)), list(sr.grid_cov(0.5, 0.5, np.deg2rad(3.0))))
        rec = lo2.onLidar(drive["stamps"][6], *drive["scans"][6])
        p = lo2.profile()
        stage.append(dict(initialize_with_load_ms=t_init, relocalize_stage_ms=p["onLidar.2.relocalize"] * 1e3, onLidar_ms=p["onLidar"] * 1e3,
                          candidates=rec["reloc_candidates"], n_for_icp=rec["n_for_icp"], relocalized=rec["relocalized"],
                          best_n_paired=rec["reloc_best_n_paired"], quality=rec["reloc_best_quality"]))
    out["driver_relocalization"] = stage[1:]   # (the first driver of the process pays the code objects)
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
