"""-m gpu: the stand-alone driver on a two-LiDAR rig (onLidarFrom, params.multiple_lidars, params.lidar_sensor_labels).

The drive is synth.make_drive(8); every sweep is split by azimuth into the half a front and the half a rear LiDAR see, each in
its own sensor frame (tests/multi_lidar_inline.py: yaws of 25 and -160 degrees, lever arms of about a metre), the rear sensor
stamped 4 ms later, the rear observation arriving first on odd scans.

Exact identity: the rig driver equals a plain onLidar run on the same text without its observations_filter_adjust_timestamps
block, fed tests/merge_ref.py's cloud of every group at the triggering stamp -- trajectories byte for byte, every record key.
One thing has to be arranged for it: the rig takes its FIRST sensor-range estimate from the first observation alone
(LidarOdometry.cpp:662, before the sensors are synchronised), a plain run from its first whole cloud.  In the identity drive
the rear sensor's first message is therefore empty (a legal source), so that both first estimates come from the same points;
after that nothing is left free.  The tracking drive has no such arrangement.

Measured on an MI355X (8 scans): ATE of the rig run 0.0893 m, of the unsplit drive through onLidar (the yardstick, same test
run) 0.0885 m; the bar 2 x 0.0885 + 0.032 = 0.2090 m is met."""
import numpy as np
import pytest

from mola_lidar_odometry_amd import synth, trajectory

import merge_ref as MR
import multi_lidar_inline as ML

pytestmark = pytest.mark.gpu
F = np.float32
N_SCANS = 8
NEW_KEYS = ("n_sensors", "sensor_labels")  # what differs by entry point: one source on onLidar, the group on onLidarFrom


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def drive():
    return synth.make_drive(N_SCANS)


def new_driver(host, text):
    lo = host.LidarOdometry(0, True)
    lo.initialize(host.Config.FromYamlText(text))
    return lo


def observations(drive, empty_first_rear=False):
    """The rig's messages in arrival order: per scan [(label, stamp, xyz in the sensor frame, per-point stamps)] x 2."""
    out = []
    for k, ((xyz, t), st) in enumerate(zip(drive["scans"], drive["stamps"])):
        halves = ML.split(xyz, t)
        if empty_first_rear and k == 0:
            halves[ML.REAR] = (np.zeros((0, 3), F), np.zeros(0, F))
        msgs = [(ML.FRONT, float(st), *halves[ML.FRONT]), (ML.REAR, float(st) + ML.REAR_DELAY, *halves[ML.REAR])]
        out.append(msgs[::-1] if k % 2 else msgs)
    return out


def feed(lo, msgs):
    return [lo.onLidarFrom(label, st, xyz, t, sensor_pose=list(ML.POSE[label].ravel())) for label, st, xyz, t in msgs]


def same_trajectory(a, b):
    return len(a) == len(b) and all(p[0] == q[0] and np.array(p[1]).tobytes() == np.array(q[1]).tobytes() for p, q in zip(a, b))


def ate(lo, drive):
    stamps = np.asarray(drive["stamps"])
    traj = lo.trajectory()
    assert len(traj) == len(stamps), "the driver lost track"
    at = [int(np.argmin(np.abs(stamps - t))) for t, _ in traj]
    est = np.array([trajectory.to44(np.array(T)) for _, T in traj])
    gt = np.stack([trajectory.to44(p) for p in drive["poses"]])
    return trajectory.ate_rmse(est, gt[at], align="origin")


def bbox_radius(xyz):
    """The driver's bounding-box radius (float norms of the two corners of the finite points' box)."""
    p = xyz[np.isfinite(xyz).all(1)]
    mx, mn = p.max(0).astype(F), p.min(0).astype(F)
    norm = lambda v: np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])  # noqa: E731
    return float(max(norm(mx), norm(mn)))


def test_rig_equals_a_plain_run_on_the_merged_clouds(host, drive):
    rig = new_driver(host, ML.pipeline(2, 0.01))
    plain = new_driver(host, ML.pipeline(1, 0.01, adjust_timestamps=False))
    assert rig.describePipeline()["timestamp_method"] == "1" and plain.describePipeline()["timestamp_method"] == "0"
    group_records = []
    for k, msgs in enumerate(observations(drive, empty_first_rear=True)):
        first, second = feed(rig, msgs)
        assert first["waiting"] and not second["waiting"] and second["n_sensors"] == 2
        assert second["sensor_labels"] == [ML.FRONT, ML.REAR] and second["timestamp"] == msgs[1][1]
        by_label = {m[0]: m for m in msgs}
        t_first = by_label[ML.FRONT][1]  # label order, not arrival order
        want = MR.merge([dict(xyz=by_label[l][2], t=by_label[l][3], pose=ML.POSE[l], method=MR.TS_MIDDLE_IS_ZERO,
                              offset=by_label[l][1] - t_first) for l in (ML.FRONT, ML.REAR)])
        assert second["n_raw"] == len(want["xyz"])
        rec = plain.onLidar(msgs[1][1], want["xyz"], want["t"])
        group_records.append(second)
        for key in rec:
            if key not in NEW_KEYS:
                assert rec[key] == second[key], (k, key, rec[key], second[key])
        assert rec["n_sensors"] == 1 and rec["sensor_labels"] == []
    assert same_trajectory(rig.trajectory(), plain.trajectory()) and len(rig.trajectory()) == N_SCANS
    assert sum(r["icp_run"] for r in group_records) == N_SCANS - 1 and any(r["twist_corrections"] for r in group_records)
    assert rig.dynamicVariables()["SENSOR_TIME_OFFSET"] == (float(drive["stamps"][-1]) + ML.REAR_DELAY) - float(drive["stamps"][-1])
    # records(): the waiting ones are there too, and hold nothing of the map
    recs = rig.records()
    assert len(recs) == 2 * N_SCANS and [r["waiting"] for r in recs] == [True, False] * N_SCANS
    assert all(r["n_map_points"] == 0 and r["n_sensors"] == 0 for r in recs[::2])
    prof = rig.profile()
    assert prof["onLidar.0.merge_sensors"] > 0 and "onLidar.0.merge_sensors" not in plain.profile()


def test_a_rig_of_one_equals_onlidar(host, drive):
    text = ML.pipeline(1, 0.01, "lidar")
    a, b = new_driver(host, text), new_driver(host, text)
    for (xyz, t), st in zip(drive["scans"][:5], drive["stamps"][:5]):
        ra = a.onLidarFrom("lidar", float(st), xyz, t)  # no pose: identity
        rb = b.onLidar(float(st), xyz, t)
        assert not ra["waiting"] and ra["n_sensors"] == 1 and ra["sensor_labels"] == ["lidar"]
        for key in rb:
            if key not in NEW_KEYS:
                assert ra[key] == rb[key], (key, ra[key], rb[key])
    assert same_trajectory(a.trajectory(), b.trajectory()) and len(a.trajectory()) == 5


def test_waiting_records_and_the_first_range_estimate(host, drive):
    lo = new_driver(host, ML.pipeline(2, 0.01))
    msgs = observations(drive)
    label, st, xyz, t = msgs[0][0]
    assert label == ML.FRONT
    r = lo.onLidarFrom(label, st, xyz, t, sensor_pose=list(ML.POSE[label].ravel()))
    assert r["waiting"] and not r["dropped"] and not r["ignored"] and not r["icp_run"] and r["n_raw"] == len(xyz)
    assert lo.trajectory() == [] and r["pose"] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    abs_min = 5.0  # absolute_minimum_sensor_range of the text
    want = max(bbox_radius(MR.transform(ML.POSE[label], xyz)), abs_min)
    assert want > 2 * abs_min and lo.dynamicVariables()["ESTIMATED_SENSOR_MAX_RANGE"] == want
    feed(lo, msgs[0][1:])
    feed(lo, msgs[1][:1])
    pose_before, n_traj = lo.records()[-2]["pose"], len(lo.trajectory())
    r = lo.records()[-1]
    assert r["waiting"] and r["pose"] == pose_before and n_traj == 1 == len(lo.trajectory())


def test_an_observation_outside_the_window_leaves_a_group_of_one(host, drive):
    lo = new_driver(host, ML.pipeline(2, 0.01))
    halves = ML.split(*drive["scans"][0])
    st = float(drive["stamps"][0])
    poses = {l: list(ML.POSE[l].ravel()) for l in ML.POSE}
    assert lo.onLidarFrom(ML.REAR, st - 0.05, *halves[ML.REAR], sensor_pose=poses[ML.REAR])["waiting"]  # 50 ms stale
    r = lo.onLidarFrom(ML.FRONT, st, *halves[ML.FRONT], sensor_pose=poses[ML.FRONT])
    assert not r["waiting"] and r["n_sensors"] == 1 and r["sensor_labels"] == [ML.FRONT] and r["n_raw"] == len(halves[ML.FRONT][0])
    assert r["first_scan"] and r["map_updated"]
    # the waiting set is empty again: the next front observation waits
    assert lo.onLidarFrom(ML.FRONT, st + 0.1, *halves[ML.FRONT], sensor_pose=poses[ML.FRONT])["waiting"]


def test_drops_and_throws(host, drive):
    lo = new_driver(host, ML.pipeline(2, 0.01))
    halves = ML.split(*drive["scans"][0])
    f, r = halves[ML.FRONT], halves[ML.REAR]
    rec = lo.onLidarFrom("camera_front", 0.0, *f)  # outside lidar_sensor_labels
    assert rec["ignored"] and not rec["waiting"] and lo.dynamicVariables().get("ESTIMATED_SENSOR_MAX_RANGE") is None
    with pytest.raises(RuntimeError, match="onLidarFrom"):
        lo.onLidar(0.0, f[0], f[1])
    # the per-label drop, with the reference's quirk: only the label that completes a group has its time recorded
    assert lo.onLidarFrom(ML.FRONT, 10.0, *f)["waiting"]
    assert not lo.onLidarFrom(ML.REAR, 10.004, *r)["waiting"]
    rec = lo.onLidarFrom(ML.FRONT, 10.0005, *f)  # 0.5 ms after the last front observation: never recorded, not dropped
    assert rec["waiting"] and not rec["dropped"]
    rec = lo.onLidarFrom(ML.REAR, 10.0045, *r)   # 0.5 ms after the rear observation that completed the group
    assert rec["dropped"] and not rec["waiting"] and len(lo.trajectory()) == 1
    with pytest.raises(RuntimeError, match="onLidarFrom"):
        lo.prefetch(np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1]))
    one = new_driver(host, ML.pipeline(1, 0.01))
    one.prefetch(np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1]))  # fine before any labelled observation
    one.onLidarFrom(ML.FRONT, 0.0, *f)
    with pytest.raises(RuntimeError, match="labelled observation"):
        one.prefetch(np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1]))
    assert one.onLidarFrom(ML.FRONT, 0.0005, *f)["dropped"]


def test_reset_and_a_second_drive_reproduce_the_first(host, drive):
    lo = new_driver(host, ML.pipeline(2, 0.01))
    msgs = observations(drive)[:4]
    for m in msgs:
        feed(lo, m)
    feed(lo, observations(drive)[4][:1])  # one observation left waiting
    first = lo.trajectory()
    lo.reset()
    assert lo.records() == [] and lo.trajectory() == []
    for m in msgs:
        a, b = feed(lo, m)
        assert a["waiting"] and not b["waiting"]  # (the waiting set and the per-label times started again)
    assert same_trajectory(lo.trajectory(), first) and len(first) == 4


def test_rig_tracks_the_drive(host, drive):
    """Every ICP good, and ATE <= 2 x yardstick + 0.032 m: the yardstick is the unsplit drive through onLidar on the same text,
    measured here; 0.032 m = 8 m/s x 4 ms, the shift that de-skewing the rear half to another reference instant allows."""
    text = ML.pipeline(2, 0.01)
    rig = new_driver(host, text)
    groups = [feed(rig, m)[1] for m in observations(drive)]
    assert all(g["n_sensors"] == 2 and g["n_raw"] == len(s[0]) for g, s in zip(groups, drive["scans"]))
    assert all(g["icp_good"] for g in groups[1:]) and groups[0]["first_scan"]
    plain = new_driver(host, ML.pipeline(1, 0.01))
    for (xyz, t), st in zip(drive["scans"], drive["stamps"]):
        plain.onLidar(float(st), xyz, t)
    yardstick, got = ate(plain, drive), ate(rig, drive)
    print(f"multi-lidar ATE: rig {got:.4f} m, unsplit yardstick {yardstick:.4f} m, bar {2 * yardstick + 0.032:.4f} m")
    assert got <= 2 * yardstick + 0.032
