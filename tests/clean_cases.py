"""The scenario of the map-cleaning tests (tests/test_clean_cpu.py, tests/test_gpu_clean.py): 20 key-frames 3 m apart along one
street of synth_city.make_city(2024), at rest, 32 rings x 600 azimuths, exact poses -- and one car-sized box added to the city per
sweep, at a position that moves: 12 m ahead of the vehicle for the first half, then across the street.  The box is a car's body: it
begins CLEARANCE above the road (what lies on the road agrees with the road in every other view and stays).  Data generation
only (mola_lidar_odometry_amd.synth / synth_city); no product code."""
import functools

import numpy as np

from mola_lidar_odometry_amd import synth, synth_city

N_FRAMES, SPACING = 20, 3.0
START = (34.0, -1.0)                 # first pose [m]: the street along y = 0, driven towards +x clear of the cars parked at its kerbs
BOX = (4.4, 1.8, 1.5)                # the mover: length, width, top [m] ...
CLEARANCE = 0.3                      # ... and where its body begins above the road
AHEAD, MOVER_Y = 12.0, -1.0          # first half: its centre this far ahead of the vehicle, in the vehicle's lane
CROSS_X, CROSS_Y = 84.0, (-15.0, 9.0)  # second half: it crosses the street along x = CROSS_X, from / to these y, before the vehicle
                                     # gets there (the vehicle passes every place the mover was seen at: views from both sides)
INFLATE = 0.05
SWEPT_ABOVE = 0.3
MAP_PARAMS = dict(voxel_size=1.0, max_points_per_voxel=20, index_mode=0, min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0,
                  ndt_min_points=4, far_voxel_metric=0)


def poses():
    return np.array([synth.pose_from_ypr([START[0] + SPACING * k, START[1], synth.SENSOR_H, 0.0, 0.0, 0.0]) for k in range(N_FRAMES)]).reshape(-1, 12)


def mover_box(k):
    """[xmin, ymin, zmin, xmax, ymax, zmax] of the mover during sweep k (world frame)."""
    l, w, h = BOX
    half = N_FRAMES // 2
    if k < half:  # driving ahead, along the street
        cx, cy, sx, sy = START[0] + SPACING * k + AHEAD, MOVER_Y, l, w
    else:         # crossing, turned across the street
        u = (k - half) / float(N_FRAMES - half - 1)
        cx, cy, sx, sy = CROSS_X, CROSS_Y[0] + u * (CROSS_Y[1] - CROSS_Y[0]), w, l
    return np.array([cx - sx / 2, cy - sy / 2, CLEARANCE, cx + sx / 2, cy + sy / 2, h], np.float32)


def to_world(T12, xyz):
    T = np.asarray(T12, np.float64).reshape(3, 4)
    return np.asarray(xyz, np.float64) @ T[:, :3].T + T[:, 3]


def in_box(world_xyz, box, grow=0.0):
    b = np.asarray(box, np.float64)
    return np.all((world_xyz >= b[:3] - grow) & (world_xyz <= b[3:] + grow), axis=1)


@functools.lru_cache(maxsize=1)
def scenario():
    """dict(poses [20, 12], sweeps: 20 float32 [n, 3] (vehicle frame), boxes [20, 6], mover: 20 bool masks)"""
    city = synth_city.make_city(2024)
    P = poses()
    sweeps, boxes, mover = [], [], []
    for k, T in enumerate(P):
        box = mover_box(k)
        rc = synth_city.Raycaster(dict(city, boxes=np.concatenate([city["boxes"], box[None]], 0)))
        xyz = np.ascontiguousarray(rc.sweep(T, np.zeros(6), rings=32, azimuths=600, seed=900 + k)[0], np.float32)
        rc.close()
        sweeps.append(xyz)
        boxes.append(box)
        mover.append(in_box(to_world(T, xyz), box, INFLATE))
    return dict(poses=P, sweeps=sweeps, boxes=np.array(boxes), mover=mover)


def keyframe_set(poses_, sweeps):
    """the dict host.write_keyframe_file / host.clean_keyframes take: every sweep the single stored layer of the single map"""
    maps = [dict(name="localmap", class_name="HashedVoxelPointCloud", params=dict(MAP_PARAMS), remove_voxels_farther_than=0.0)]
    frames = [dict(timestamp=2000.0 + k, pose=[float(v) for v in T], cov=[0.0] * 36, twist=None, layers=[(0, xyz)])
              for k, (T, xyz) in enumerate(zip(poses_, sweeps))]
    return dict(maps=maps, frames=frames)


def in_swept_volume(world_xyz, boxes):
    """inside any of the sweeps' boxes, above SWEPT_ABOVE"""
    m = np.zeros(len(world_xyz), bool)
    for b in boxes:
        m |= in_box(world_xyz, b)
    return m & (world_xyz[:, 2] > SWEPT_ABOVE)
