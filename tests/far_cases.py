"""The inputs of tests/dense_cases.py moved far from the origin: maps and poses shifted by D in float64 and rounded once to
fp32, the scans left in their sensor frames.  Host arrays only, no GPU.

An odometry run leaves the origin by kilometres and maps arrive in tile coordinates tens of kilometres out; every margin of
the searches (axis_gaps' 1e-6 * (|c| + 2) * vs, the * 0.9999f tests, the radius search's 2.4e-7 * |result|) was argued to scale
with the coordinate's magnitude.  tests/test_far_cpu.py shows on the references alone that they stay sound out here;
tests/test_gpu_far_origin.py holds every device route to them.

OFFSETS [m] and the fp32 spacing they leave in x / y:
  D1  a long drive           4.9e-4 / 2.4e-4 m
  D2  tile coordinates       3.9e-3 / 2.0e-3 m
  D3  1/32 m in x and y: the room's 3 cm grid snaps onto the fp32 lattice, so equal distances abound; |p| / vs is 8.2e5 at the
      0.5 m voxel of `capped`, still inside the key range (|p / vs| < 1e6)."""
import numpy as np

import dense_cases as dc

D1 = (4099.3, -2051.7, 3.1)
D2 = (-52431.7, 30011.3, -12.4)
D3 = (4.1e5, -3.9e5, 50.0)
ORIGIN = (0.0, 0.0, 0.0)
OFFSETS = {"D1": D1, "D2": D2, "D3": D3}
KEY_SAFE = 9.0e5   # a case is used at an offset only while |p| / cell stays below this on every axis (the key range ends at 1e6)

# Every voxel size of dense_cases.Inputs is a power of two: voxel planes are fp32 numbers and p * (1 / vs) is exact, so a
# search's slab bounds are exact at any distance.  A voxel of 0.7 m is not: fl(1 / 0.7) * fl(0.7) != 1, a record's voxel and the
# slab (float)v * vs disagree by ulps of the COORDINATE near every voxel face, which is what axis_gaps' scaled margin absorbs.
# `room07`: the dense room under that voxel (uncapped: dozens to hundreds of records per voxel).
VS_ODD = 0.7


def shift_points(pts, D):
    """pts + D in float64, rounded once to fp32"""
    return np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3) + np.asarray(D, np.float64), np.float32)


def shift_pose(T, D):
    """the pose (12 doubles, row-major 3 x 4) with D added to its translation"""
    T = np.array(T, np.float64).reshape(-1)[:12].copy()
    T[3::4] += np.asarray(D, np.float64)
    return T


def usable(D, cell, reach=8.0):
    """True while every coordinate within `reach` metres of D keeps |p| / cell < KEY_SAFE"""
    return bool((np.abs(np.asarray(D, np.float64)).max() + reach) / float(cell) < KEY_SAFE)


def far_inputs(D):
    """A dense_cases.Inputs whose maps, queries, T_gt, T0, T1 and T_kf are shifted by D; scan and keyframe stay in their sensor
    frames.  `mixed` is thinned AFTER the shift (its voxel classes are a property of where the voxel faces fall).  One map more
    than at the origin: room07, the room under the 0.7 m voxel."""
    inp = dc.Inputs()
    room = shift_points(inp.maps["room"][0], D)
    inp.maps = {"room": (room, dc.VS, 0, 0.0), "mixed": (dc.thin_odd_voxels(room), dc.VS, 0, 0.0),
                "centres": (shift_points(inp.maps["centres"][0], D), dc.VS, 0, 0.0), "room_clear": (room, dc.VS, 0, dc.CLEARANCE),
                "capped": (np.ascontiguousarray(room[::3]), 0.5, 20, 0.0), "room07": (room, VS_ODD, 0, 0.0)}
    inp.queries = shift_points(inp.queries, D)
    for k in ("T_gt", "T0", "T1", "T_kf"):
        setattr(inp, k, shift_pose(getattr(inp, k), D))
    inp.D = tuple(float(v) for v in D)
    return inp


def spacing(D):
    """the fp32 spacing at D, per axis"""
    return np.spacing(np.abs(np.asarray(D, np.float32)))


SINGLE_MAPS = ("room", "mixed")
SINGLE_SIZES = (129, 2561)


def ulps(a, b):
    """|a - b| in units of the fp32 spacing at b, elementwise"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
