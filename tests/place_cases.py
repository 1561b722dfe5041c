"""The scenario of tests/test_odometry_place.py, shared with the CPU checks of tests/test_place_cpu.py: key-frame poses along the
street of synth.make_scene(4242, 120, 160), their sweeps, and query sweeps taken beside three of them under an arbitrary yaw.
Data generation only (mola_lidar_odometry_amd.synth); the layers a key-frame stores come from whoever runs the filter chain."""
import numpy as np

from mola_lidar_odometry_amd import synth

SCENE = (4242, 120.0, 160)
KF_X = [-105.0 + 10.0 * k for k in range(12)]   # 12 key-frame poses, 10 m apart: x = -105 .. 5
SENSOR_Z = synth.SENSOR_H
# (key-frame index, yaw [rad], offset across the street [m]); all 0.4 m further along the street
QUERIES = [(2, 0.3, 0.3), (6, 2.4, -0.5), (9, -1.6, 0.4)]
# The street is self-similar: with the odometry's own acceptance (min_icp_goodness 0.25) the reference accepts wrong places too
# (measured on the CPU: quality 0.69-0.87 at wrong places, 0.98-1.0 at the right ones).  Every run of the scenario therefore asks
# for 0.9 (MOLA_MINIMUM_ICP_QUALITY), the true places and the far one alike.
MIN_QUALITY = "0.9"
GT_BOUND = 0.1   # [m] per axis: the bound of test_odometry_localize.py::test_relocalization_from_a_coarse_pose
FAR_QUERY = (100.0, 0.0, SENSOR_Z, 0.7, 0.0, 0.0)   # the other end of the scene: 95 m beyond the last key-frame


def scene():
    return synth.make_scene(*SCENE)


def kf_pose(k):
    """(x, y, z, yaw, pitch, roll) of key-frame k"""
    return np.array([KF_X[k], 0.5, SENSOR_Z, 0.0, 0.0, 0.0])


def query_pose(q):
    k, yaw, across = QUERIES[q]
    return kf_pose(k) + np.array([0.4, across, 0.0, yaw, 0.0, 0.0])


def sweep(sc, pose_ypr, seed):
    """one 32 x 600 sweep at rest (zero twist): (xyz float32 [n, 3], t float32 [n])"""
    return synth.make_sweep(sc, synth.pose_from_ypr(pose_ypr), np.zeros(6), rings=32, azimuths=600, seed=seed)


def kf_sweeps(sc):
    return [sweep(sc, kf_pose(k), 100 + k) for k in range(len(KF_X))]


def query_sweeps(sc):
    return [sweep(sc, query_pose(q), 200 + q) for q in range(len(QUERIES))]


def pipeline_text(path):
    """the pipeline file with a smaller candidate search: two key-frames kept, +-1.5 m around each (the queries stand 0.5-0.7 m
    from their key-frame); what the device driver and the reference both read"""
    txt = open(path).read()
    assert txt.count("  place_top_k: 4\n") == 1 and txt.count("  place_sigma_xy: 1.0\n") == 1
    return txt.replace("  place_top_k: 4\n", "  place_top_k: 2\n").replace("  place_sigma_xy: 1.0\n", "  place_sigma_xy: 0.5\n")
