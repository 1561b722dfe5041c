"""Wall time of mh_occmap_insert_frames against the loop of mh_occmap_insert it is defined by, on the same frames, and of
mh_occmap_project_grid.  Two sessions: the 12 key-frames of the 10 m x 8 m room of tests/occgrid_ref.py (720 points each,
resolution 0.05 m) and the 20 key-frames of the street of tests/clean_cases.py (synth_city, about 18 000 points each, resolution
0.2 m), both at the library's pass sizes.  Host clock around calls that end in a device synchronise (both routes read counters
back); warm-ups first, then the median of the repeats, the two routes alternating.  The loop's scans are uploaded before its clock
starts; the batched call's host arrays are uploaded inside it.  Run under `rocprofv3 --kernel-trace --stats` for the time of the
key kernel (k_occf_keys): the keys it wrote are printed here (n_keys).  Usage: python tools/occgrid_time.py [room|street ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from mola_lidar_odometry_amd import capi, capi_occgrid as og


def sessions(which):
    if "room" in which:
        import occgrid_ref as G
        yield "room", G.room_session()[0], 0.05, 3, 15
    if "street" in which:
        import clean_cases as cc
        sc = cc.scenario()
        yield "street", list(zip(sc["sweeps"], sc["poses"])), 0.2, 1, 5


ctx = capi.Context(0)
for name, frames, res, warm, reps in sessions(sys.argv[1:] or ["room", "street"]):
    scans = [capi.Scan(ctx, xyz) for xyz, _ in frames]
    ctx.synchronize()

    def loop():
        m = capi.OccMap(ctx, resolution=res)
        ctx.synchronize()
        t0 = time.perf_counter()
        keys = 0
        for s, (_, T) in zip(scans, frames):
            m.insert(s, T, 0.0)
            keys += m.info().n_keys
        dt = time.perf_counter() - t0
        return dt, m, keys

    def batched():
        m = capi.OccMap(ctx, resolution=res)
        ctx.synchronize()
        t0 = time.perf_counter()
        og.insert_frames(m, frames)
        i = m.info()
        dt = time.perf_counter() - t0
        return dt, m, int(i.n_keys)

    tl, tb, tp = [], [], []
    for rep in range(warm + reps):
        (a, ma, ka), (b, mb, kb) = loop(), batched()
        assert ka == kb and all(np.array_equal(x, y) for x, y in zip(ma.download(), mb.download()))
        lo, hi, n = og.index_bounds(mb)
        t0 = time.perf_counter()
        g = og.project_grid(mb, int(lo[0]) - 2, int(lo[1]) - 2, int(hi[0] - lo[0]) + 5, int(hi[1] - lo[1]) + 5, int(lo[2]), int(hi[2]))
        p = time.perf_counter() - t0
        info = mb.info()
        ma.close(), mb.close()
        if rep >= warm:
            tl.append(a), tb.append(b), tp.append(p)
    ms = lambda t: round(1e3 * float(np.median(t)), 3)
    print(json.dumps(dict(session=name, frames=len(frames), points=int(sum(len(x) for x, _ in frames)), resolution=res, n_keys=kb,
                          key_chunks=int(info.n_passes), cells=int(n), grid=list(g.shape), loop_ms=ms(tl), batched_ms=ms(tb),
                          project_ms=ms(tp), speedup=round(float(np.median(tl) / np.median(tb)), 2),
                          loop_ms_all=[round(1e3 * t, 2) for t in tl], batched_ms_all=[round(1e3 * t, 2) for t in tb])))
