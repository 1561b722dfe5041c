"""Recorded sessions moved far from the origin, for tests/test_far_session_cpu.py and tests/test_gpu_far_session.py: the key-frame
sets, sweeps and frame lists of the near-origin tests (clean_cases, live_cases, occgrid_cases, elev_cases, test_gpu_insert_frames)
with their POSES moved and their points left in the sensor frames.  Host arrays only: no GPU, no product code.

Two ways to move a session.  A pure shift (far_cases.shift_pose) adds D to every translation and leaves every rotation entry as it
was: relative poses and distances between key-frames change in their last bits at most.  turned(T, yaw, D) premultiplies the pose
by the world transform (Rz(yaw), D): with yaw = 0.7 every entry of R and every relative pose becomes a rounded number, and the ties
of the neighbour rule (key-frames 3 m apart under a 30 m limit) are decided by the last bit of a sum of squares.

An input is used at an offset only while far_cases.usable(D, cell, reach) holds (the key range ends at |p / cell| = 1e6); the pairs
of offset and cell size below are the ones the tests use.  limit_frames() is the one input that leaves the range on purpose: a pose
40 cells short of 1e6 with points up to 80 cells around it."""
import numpy as np

import far_cases as fc
from far_cases import KEY_SAFE, OFFSETS, ORIGIN, shift_pose, usable  # noqa: F401  (re-exported: the tests name them through this module)

F = np.float32
YAW = 0.7
OCC_CASES = [("D1", 0.05), ("D2", 0.25), ("D3", 0.5)]     # (offset, resolution) of the occupancy map
ELEV_CASES = [("D2", 0.2), ("D3", 0.5)]                   # ... of the elevation map, both turned by YAW
FILE_RESOLUTIONS = (0.05, 0.1, 0.2, 0.25, 0.5, 0.7)
LIMIT_SHORT, LIMIT_REACH = 40, 80                         # cells: the limit pose lies this far short of 1e6, its points reach this far


def turned(T, yaw=YAW, D=ORIGIN):
    """(Rz(yaw), D) * T in float64: the pose (12 doubles, row-major 3 x 4) seen from a world frame turned about z and shifted"""
    M = np.array(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    c, s = np.cos(float(yaw)), np.sin(float(yaw))
    W = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    out = np.empty((3, 4))
    out[:, :3] = W @ M[:, :3]
    out[:, 3] = W @ M[:, 3] + np.asarray(D, np.float64)
    return out.reshape(12)


def move_pose(T, D=ORIGIN, yaw=None):
    """shifted by D (yaw None: the rotation keeps every bit) or turned by yaw and shifted by D"""
    return shift_pose(T, D) if yaw is None else turned(T, yaw, D)


def move_poses(poses, D=ORIGIN, yaw=None):
    return np.array([move_pose(T, D, yaw) for T in poses]).reshape(-1, 12)


def move_frames(frames, D=ORIGIN, yaw=None):
    """(xyz, T) pairs: the same arrays under moved poses"""
    return [(xyz, move_pose(T, D, yaw)) for xyz, T in frames]


def move_keyframe_set(kfset, D=ORIGIN, yaw=None):
    """the dict the host takes (maps, frames): every frame's pose moved, everything else as it was"""
    return dict(maps=kfset["maps"], frames=[dict(f, pose=[float(v) for v in move_pose(f["pose"], D, yaw)]) for f in kfset["frames"]])


def window_of(frames, resolution, margin=0):
    """(x0, y0, nx, ny) that holds every finite point of the frames, wherever they lie (elev_cases.window_of looks no farther than
    10 km); computed in float64, one cell of slack for the rounding; a negative margin cuts points off on every side"""
    with np.errstate(all="ignore"):
        pts = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) @ np.asarray(T).reshape(3, 4)[:, :3].T + np.asarray(T).reshape(3, 4)[:, 3]
                              for x, T in frames if len(x)])
        pts = pts[np.isfinite(pts).all(axis=1)]
    lo = np.floor(pts[:, :2].min(axis=0) / resolution).astype(np.int64) - 1 - margin
    hi = np.floor(pts[:, :2].max(axis=0) / resolution).astype(np.int64) + 1 + margin
    return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)


def limit_frames(resolution, sizes=(257, 65, 0, 64), seed=9, height=0.2):
    """Frames at the end of the key range: every pose has x = (1e6 - LIMIT_SHORT) * resolution (y, z and yaw scattered), the points
    lie within LIMIT_REACH cells of the vehicle, so some of them have |x / resolution| >= 1e6 and most do not."""
    rng = np.random.default_rng(seed)
    reach = LIMIT_REACH * float(resolution)
    out = []
    for n in sizes:
        xyz = rng.uniform(-reach, reach, (n, 3)).astype(F)
        xyz[:, 2] *= height
        yaw = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(yaw), np.sin(yaw)
        x, y, z = (1.0e6 - LIMIT_SHORT) * float(resolution), rng.uniform(-3, 3) * reach, rng.uniform(-0.1, 0.1) * reach
        out.append((xyz, np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, z], np.float64)))
    return out


def composed(xyz, T):
    """(float)(((T0 x + T1 y) + T2 z) + T3) per row: the product of two doubles and their sums, rounded to float once.  Written out
    entry by entry for the exhaustive counts of the tests (the restatements have their own)."""
    p = np.asarray(xyz, F).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1)[:12]
    out = np.empty((len(p), 3), F)
    for r in range(3):
        out[:, r] = ((T[4 * r] * p[:, 0] + T[4 * r + 1] * p[:, 1]) + T[4 * r + 2] * p[:, 2]) + T[4 * r + 3]
    return out


def words_differing(a, b):
    """how many entries of two lists of equally shaped arrays differ"""
    return int(sum((np.asarray(x) != np.asarray(y)).sum() for x, y in zip(a, b)))


assert all(usable(OFFSETS[name], res, 20.0) for name, res in OCC_CASES + ELEV_CASES)
assert all(usable(D, 1.0, 200.0) for D in OFFSETS.values())     # the 1 m voxel of the point maps, a street of 100 m with 60 m of range
assert fc.ORIGIN == (0.0, 0.0, 0.0)
