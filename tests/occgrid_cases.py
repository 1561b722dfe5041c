"""Frames for the tests of mh_occmap_insert_frames (tests/test_occgrid_cpu.py, tests/test_gpu_occgrid.py): seeded random key-frames
with short rays (the restatement walks every ray), the hand-made ray shapes, and the clamp case that tells a fold in frame order
from a sum of counts.  Everything is (xyz float32 [n, 3], T [12]) pairs."""
import numpy as np

RES = 0.05
I12 = np.eye(4)[:3].reshape(12)


def pose(x=0.0, y=0.0, z=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, z], np.float64)


def random_frames(sizes, seed, reach=1.5, spread=0.6):
    """One frame per entry of `sizes`: points within `reach` of the vehicle, poses scattered by `spread` with a yaw each."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        xyz = rng.uniform(-reach, reach, (n, 3)).astype(np.float32)
        xyz[:, 2] *= 0.2
        out.append((xyz, pose(*rng.uniform(-spread, spread, 3) * np.array([1, 1, 0.1]), yaw=rng.uniform(-np.pi, np.pi))))
    return out


def ray_shapes():
    """Rays of M = 0 (the end cell is the origin cell), 1, 2 and about 300 cells, along every axis, along diagonals, and to points
    that lie exactly on cell faces (multiples of the resolution as fp32 computes them)."""
    c = RES / 2
    f = np.float32
    pts = [(c, c, c), (0.01, 0.04, 0.02),                                    # M = 0
           (RES + c, c, c), (c, -c, c), (c, c, RES + c),                     # M = 1
           (2 * RES + c, c, c), (-RES - c, 2 * RES + c, c), (c, c, -RES - c),  # M = 2
           (15.0 + c, c, c), (c, -15.0 + c, c), (c, c, 15.0 + c),            # about 300 cells, axis-aligned
           (15.0 + c, 15.0 + c, c), (-15.0 + c, 15.0 + c, 15.0 + c), (15.0 + c, 7.3, -3.1), (-2.0, -14.9, 9.9)]  # ... and diagonal
    faces = [(float(f(k) * f(RES)), float(f(j) * f(RES)), float(f(i) * f(RES)))
             for k, j, i in [(1, 0, 0), (0, 1, 0), (2, 2, 0), (-1, 3, 1), (7, -7, 0), (40, 0, 0), (-3, -3, -3), (20, 10, 5)]]
    a = np.array(pts + faces, np.float32)
    return [(a, I12.copy()), (a[::-1].copy(), pose(0.31, -0.17, 0.02, 0.4)), (a[::2].copy(), pose(-1.0 * RES, 2.0 * RES, 0.0, np.pi / 2))]


# ---- the clamp case.  From a pose at the origin (origin cell (0, 0, 0)) the point HIT ends in the wall cell W = (40, 0, 0), the point
# THROUGH ends in (60, 0, 0) and its ray passes through W.  With lidar2d.yaml's integers (l_hit = l_miss = 14, l_min = -47,
# l_max = 47): six hit frames (14, 28, 42, 47, 47, 47: clamped at l_max), eight look-through frames (33, 19, 5, -9, -23, -37, -47,
# -47: clamped at l_min), one more hit: W ends at -47 + 14 = -33.  The summed counts applied as ONE insert give, counted: h = 7,
# m = 8 -> min(47, 98) = 47 -> max(-47, 47 - 112) = -47; once: a hit -> 14.  Both differ from -33.
WALL = (40, 0, 0)
HIT = np.array([[40 * RES + RES / 2, RES / 2, RES / 2]], np.float32)
THROUGH = np.array([[60 * RES + RES / 2, RES / 2, RES / 2]], np.float32)
WALL_IN_ORDER = -33
WALL_SUMMED = {"counted": -47, "once": 14}


def clamp_frames():
    return [(HIT, I12.copy())] * 6 + [(THROUGH, I12.copy())] * 8 + [(HIT, I12.copy())]


def clamp_frames_once_own():
    """The once rule's own order case: frames that BOTH hit W and look through it (the hit wins inside a frame), between frames that
    only look through it."""
    both = np.concatenate([HIT, THROUGH, THROUGH])
    return [(THROUGH, I12.copy())] * 2 + [(both, I12.copy())] * 5 + [(THROUGH, I12.copy())] * 3 + [(both, I12.copy())]


def wild_frames(seed=5):
    """Frames with non-finite points and points outside the key range (|p / resolution| >= 1e6: these are counted) among good ones."""
    out = random_frames([65, 64, 33], seed)
    for k, (xyz, T) in enumerate(out):
        xyz[3] = (np.nan, 0.1, 0.1)
        xyz[7] = (0.2, np.inf, 0.0)
        xyz[11 + k] = (6.0e4, 0.0, 0.0)
        xyz[20] = (0.0, -7.0e4, 1.0)
    return out
