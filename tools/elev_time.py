"""Wall time of the calls of include/molahip_elevation.h on a session of a few hundred key-frames: mh_elev_bounds_frames,
mh_elev_add_frames, mh_elev_mark_frames and the two relief calls of build_traversability_map, at 0.20 m.  The session is synthetic:
one sweep of 64 rings x 1 563 azimuths (100 032 points, ring after ring, as a spinning lidar delivers them) over a rolling ground
with walls on both sides, seen from FRAMES poses 2 m apart along a gentle curve.  Every call is timed twice over: with the frames in
host memory (packed into the page-locked mirror and uploaded inside the clock, as build_traversability_map does it) and with the
frames resident on the device (MH_MEM_DEVICE: the passes alone).  Host clock around calls that end in a device synchronise; warm-ups
first, then the median of the repeats.  Usage: python tools/elev_time.py [FRAMES [max_range]]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from mola_lidar_odometry_amd import capi, capi_elevation as ce

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 300
MAX_RANGE = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
RES, WARM, REPS = 0.2, 1, 5


def sweep(seed=1):
    """float32 [100 032, 3], vehicle frame, sensor 1.8 m over the ground: ring k looks down by 0.6 .. 25 degrees"""
    rng = np.random.default_rng(seed)
    down = np.deg2rad(np.linspace(25.0, 0.6, 64))[:, None]
    az = np.linspace(-np.pi, np.pi, 1563, endpoint=False)[None, :]
    r = np.minimum(1.8 / np.tan(down), 80.0) * np.ones_like(az)
    x, y = r * np.cos(az), r * np.sin(az)
    z = -r * np.tan(down) + 0.05 * np.sin(0.3 * x) + rng.normal(0, 0.01, x.shape)
    wall = np.abs(y) > 12.0                                   # walls 12 m to either side: the rings end on them
    s = np.where(wall, 12.0 / np.maximum(np.abs(y), 1e-9), 1.0)
    x, y, z = x * s, y * s, np.where(wall, z * s + rng.uniform(0, 1.5, x.shape), z)
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32))


def poses(n):
    out = []
    for k in range(n):
        yaw = 0.004 * k
        c, s = np.cos(yaw), np.sin(yaw)
        out.append(np.array([c, -s, 0, 2.0 * k * np.cos(0.002 * k), s, c, 0, 2.0 * k * np.sin(0.002 * k), 0, 0, 1, 0.02 * k], np.float64))
    return out


def timed(fn, ctx):
    ts = []
    for rep in range(WARM + REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if rep >= WARM:
            ts.append(dt)
    return out, ts


ctx = capi.Context(0)
xyz = sweep()
Ts = poses(FRAMES)
n_points = FRAMES * len(xyz)
host_frames = [(xyz, T) for T in Ts]
dev = [torch.from_numpy(np.ascontiguousarray(xyz[:, k])).cuda() for k in range(3)]
torch.cuda.synchronize()
dev_frames = [(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(xyz), T) for T in Ts]
ms = lambda t: round(1e3 * float(np.median(t)), 3)
row = dict(frames=FRAMES, points=n_points, resolution=RES, max_range=MAX_RANGE)
planes = {}
L = ce.lib()
for name, frames, mem in (("host", host_frames, capi.MEM_HOST), ("device", dev_frames, capi.MEM_DEVICE)):
    keep, arr, n_arr = ce._table(frames, mem)               # the frame table once: the clocks below hold the library's calls alone
    add_frames = lambda m: capi._chk(L.mh_elev_add_frames(m._h, arr, n_arr, mem, 0))
    mark_frames = lambda m: capi._chk(L.mh_elev_mark_frames(m._h, arr, n_arr, mem, 0))
    lo, hi, n_in = ce.bounds_frames(ctx, frames, RES, MAX_RANGE, mem=mem)
    two, cnt = np.zeros(2, np.int32), ce.C.c_uint64(0)
    _, tb = timed(lambda: capi._chk(L.mh_elev_bounds_frames(ctx._h, arr, n_arr, mem, RES, MAX_RANGE, 0, two.ctypes.data_as(ce._I32P),
                                                            two.ctypes.data_as(ce._I32P), ce.C.byref(cnt))), ctx)
    nx, ny = int(hi[0] - lo[0]) + 5, int(hi[1] - lo[1]) + 5
    m = ce.ElevMap(ctx, resolution=RES, max_range=MAX_RANGE, x0=int(lo[0]) - 2, y0=int(lo[1]) - 2, nx=nx, ny=ny)
    _, ta = timed(lambda: (m.clear(), add_frames(m)), ctx)                  # (the clear is a fill of the four planes: timed below)
    _, tc = timed(lambda: m.clear(), ctx)
    add_frames(m)
    _, tm = timed(lambda: mark_frames(m), ctx)              # (marking again changes the counts, not the work)
    _, tr = timed(lambda: (m.relief(1, 2), m.relief(2, 2)), ctx)
    info = m.info()
    m.clear()
    add_frames(m)
    mark_frames(m)
    planes[name] = m.download()
    add = np.median(ta) - np.median(tc)
    row[name] = dict(bounds_ms=ms(tb), add_ms=round(1e3 * add, 3), clear_ms=ms(tc), mark_ms=ms(tm), two_reliefs_ms=ms(tr),
                     add_gpoints_per_s=round(n_points / add / 1e9, 2), mark_gpoints_per_s=round(n_points / float(np.median(tm)) / 1e9, 2),
                     add_ms_all=[round(1e3 * (t - np.median(tc)), 2) for t in ta], mark_ms_all=[round(1e3 * t, 2) for t in tm])
    row.update(grid=[ny, nx], n_in=n_in, counted=int(info.n_counted), left_out=int(info.n_left_out),
               cells_known=int((planes[name][1] >= 2).sum()), max_count=int(planes[name][1].max()))
    m.close()
assert all(np.array_equal(a, b) for a, b in zip(planes["host"], planes["device"]))
print(json.dumps(row))
