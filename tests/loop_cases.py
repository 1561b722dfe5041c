"""The scenario of the loop-closure tests (tests/test_loop_cpu.py, tests/test_gpu_loop.py): one block of synth_city's street grid
driven once, then 36 m of its first street again, as 66 key-frames 6 m apart whose recorded poses drift away from the truth.
Data generation only (mola_lidar_odometry_amd.synth / synth_city); no product code."""
import functools

import numpy as np
import pytest

from mola_lidar_odometry_amd import synth, synth_city

ROUTE = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 0), (1, 0)]   # one 360 m block, then the first street again
SPACING, LAST_ARC = 6.0, 396.0                              # a frame every 6.0 m of arc: 0, 6, ..., 390 -> 66 frames
LATERAL = (0.4, -0.3, 340.0)                                # [m] left of the path before 340 m of arc, after it
SCALE = 1.004                                               # drift: every step's translation scaled ...
DRIFT_ROTVEC = np.array([0.0, 0.0004, 0.0012])              # ... and followed by Exp_SO3 of this
MAP_PARAMS = dict(voxel_size=1.0, max_points_per_voxel=20, index_mode=0, min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0,
                  ndt_min_points=4, far_voxel_metric=0)     # the `localmap` of pipelines/lidar3d-default-hip.yaml on a 1 m grid
OPTIONS = "\nloop_closure:\n  min_travel_between_closures: 18\n"   # about four verifications; the rest are the defaults


def to44(T12):
    return np.vstack([np.asarray(T12, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def to12(T44):
    return np.ascontiguousarray(np.asarray(T44, np.float64)[:3].reshape(12))


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / (th * th) * (W @ W)


def ground_truth():
    """[66, 12] poses on the path of ROUTE (the module's route is swapped for the call, no file is edited)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(synth_city, "ROUTE", ROUTE)
        px, py, ph, _ = synth_city._planned_path(0.1)
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(px), np.diff(py)))])
    assert arc[-1] > LAST_ARC
    out = []
    for a in np.arange(0.0, LAST_ARC, SPACING):
        k = int(np.searchsorted(arc, a))
        lat = LATERAL[0] if a < LATERAL[2] else LATERAL[1]
        h = ph[k]
        out.append(synth.pose_from_ypr([px[k] - lat * np.sin(h), py[k] + lat * np.cos(h), synth.SENSOR_H, h, 0.0, 0.0]))
    return np.array(out).reshape(-1, 12)


def drifted(gt):
    """est_0 = gt_0, est_k = est_{k-1} . D_k . E: D_k the true step with its translation scaled, E a small constant rotation"""
    E = np.eye(4)
    E[:3, :3] = exp_so3(DRIFT_ROTVEC)
    est = [to44(gt[0])]
    for k in range(1, len(gt)):
        D = np.linalg.inv(to44(gt[k - 1])) @ to44(gt[k])
        D[:3, 3] *= SCALE
        est.append(est[-1] @ D @ E)
    return np.array([to12(T) for T in est])


@functools.lru_cache(maxsize=1)
def scenario():
    """dict(gt [66, 12], est [66, 12], sweeps: 66 float32 [n, 3] arrays (32 rings x 600 azimuths at rest, seed 500 + n))"""
    gt = ground_truth()
    rc = synth_city.Raycaster(synth_city.make_city(2024))
    sweeps = [np.ascontiguousarray(rc.sweep(T, np.zeros(6), rings=32, azimuths=600, seed=500 + n)[0], np.float32) for n, T in enumerate(gt)]
    rc.close()
    return dict(gt=gt, est=drifted(gt), sweeps=sweeps)


def keyframe_set(poses, sweeps):
    """the dict host.write_keyframe_file / host.close_loops take: every sweep the single stored layer of the single map"""
    maps = [dict(name="localmap", class_name="HashedVoxelPointCloud", params=dict(MAP_PARAMS), remove_voxels_farther_than=0.0)]
    frames = [dict(timestamp=1000.0 + k, pose=[float(v) for v in T], cov=[0.0] * 36, twist=None, layers=[(0, xyz)])
              for k, (T, xyz) in enumerate(zip(poses, sweeps))]
    return dict(maps=maps, frames=frames)


def position_errors(poses, gt):
    """|t_k - t_k(truth)| per frame"""
    return np.linalg.norm(np.asarray(poses).reshape(-1, 3, 4)[:, :, 3] - np.asarray(gt).reshape(-1, 3, 4)[:, :, 3], axis=1)


def relative(Tj, Ti):
    """T_j^-1 T_i as 12 values"""
    return to12(np.linalg.inv(to44(Tj)) @ to44(Ti))
