"""The run behind profiles/multi_lidar.md: a two-LiDAR rig drive (tests/multi_lidar_inline.py: 2 x 9600 points per group)
through onLidarFrom, then one unsplit 19 200-point scan through onLidar on the same text (the rig path adjusts its stamps in
the merge and never launches k_pp_tminmax_b).  Prints the host stage times per group.  For kernel durations run it under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o multi_lidar -- python tools/multi_lidar_profile.py
alone (no counters, no other tracing)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mola_lidar_odometry_amd import _mp2p_icp_hip as H, synth  # noqa: E402
import multi_lidar_inline as ML  # noqa: E402

N_SCANS = 12
drive = synth.make_drive(N_SCANS)
rig = H.LidarOdometry(0, True)
rig.initialize(H.Config.FromYamlText(ML.pipeline(2, 0.01)))
groups = 0
for k, ((xyz, t), st) in enumerate(zip(drive["scans"], drive["stamps"])):
    halves = ML.split(xyz, t)
    msgs = [(ML.FRONT, float(st)), (ML.REAR, float(st) + ML.REAR_DELAY)]
    if k == 2:
        base = dict(rig.profile())  # (steady state from here: the buffers have their sizes)
        groups = 0
    for label, stamp in (msgs[::-1] if k % 2 else msgs):
        r = rig.onLidarFrom(label, stamp, *halves[label], sensor_pose=list(ML.POSE[label].ravel()))
    assert r["n_sensors"] == 2 and (k == 0 or r["icp_good"])
    groups += 1
prof = {k: v - base.get(k, 0.0) for k, v in rig.profile().items()}
plain = H.LidarOdometry(0, True)
plain.initialize(H.Config.FromYamlText(ML.pipeline(1, 0.01)))
plain.onLidar(float(drive["stamps"][0]), *drive["scans"][0])
print(json.dumps(dict(groups=groups, points_per_group=int(r["n_raw"]),
                      merge_sensors_us_per_group=1e6 * prof["onLidar.0.merge_sensors"] / groups,
                      upload_raw_us_per_group=1e6 * prof["onLidar.0.upload_raw"] / groups,
                      onLidar_us_per_group=1e6 * prof["onLidar"] / groups)))
