"""Wall time of the place-recognition entry points: describing K frames of 10 k points in a loop of mh_place_describe + mh_place_db_add
against ONE mh_place_db_add_frames (host arrays, device arrays), and mh_place_search over 10^3 .. 10^6 stored descriptors at
20 x 64.  Host clock around calls that block until their output is there; one warm-up, then the median of 5, the routes
alternating.  The loop's scans are uploaded before the clock starts (a driver's layers are on the device already); the batched
call's host arrays are uploaded inside it.  With --numpy the restatement of tests/place_ref.py is timed on the CPU instead (no GPU
needed): one describe of 10 k points, one search over 10^3 descriptors.
Usage: python tools/place_time.py [--numpy] [K ...]   (default 200 1000)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

N = 10_000
PARAMS = dict(n_rings=20, n_sectors=64, min_range=1.0, max_range=80.0, z_min=-3.0, z_max=27.0)
args = [a for a in sys.argv[1:] if a != "--numpy"]


def frame(rng):
    """a sweep-like layer: points within 60 m of the vehicle, mostly near the ground"""
    r = 60.0 * np.sqrt(rng.uniform(0.0, 1.0, N))
    a = rng.uniform(0.0, 2 * np.pi, N)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.normal(0.0, 1.5, N)], 1).astype(np.float32)


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


if "--numpy" in sys.argv:
    import place_ref as pr
    rng = np.random.default_rng(1)
    xyz = frame(rng)
    stored = rng.integers(0, 256, (1000, 20, 64), dtype=np.uint8)
    q = pr.describe(xyz, **PARAMS)
    out = dict(describe_10k_points_ms=median_ms(lambda: pr.describe(xyz, **PARAMS)), search_1000_descriptors_ms=median_ms(lambda: pr.search(stored, q), 3))
    print(json.dumps({"place_time_numpy": out}))
    sys.exit(0)

import torch
from mola_lidar_odometry_amd import capi

ctx = capi.Context(0)
cp = capi.place_params(**PARAMS)
out = {"describe": {}, "search": {}}
for K in [int(a) for a in args] or [200, 1000]:
    rng = np.random.default_rng(K)
    frames = [frame(rng) for _ in range(K)]
    scans = [capi.Scan(ctx, xyz) for xyz in frames]
    dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(frames).T)).to("cuda:0")  # [3, K*N]
    torch.cuda.synchronize()
    ctx.synchronize()
    table = [(dev[0].data_ptr() + 4 * k * N, dev[1].data_ptr() + 4 * k * N, dev[2].data_ptr() + 4 * k * N, N) for k in range(K)]
    probe = capi.place_describe(scans[K // 2], cp)

    def run(fill):
        db = capi.PlaceDB(ctx, cp)
        ctx.synchronize()
        t0 = time.perf_counter()
        fill(db)
        dt = time.perf_counter() - t0
        m = db.search(probe)
        assert len(db) == K and m["dist"][K // 2] == 0 and m["shift"][K // 2] == 0
        db.close()
        return dt

    def loop(db):
        for s in scans:
            db.add(capi.place_describe(s, cp))

    tl, tb, td = [], [], []
    for rep in range(6):
        a, b, c = run(loop), run(lambda db: db.add_frames(frames)), run(lambda db: db.add_frames_device(table))
        if rep:
            tl.append(a); tb.append(b); td.append(c)
    row = dict(frames=K, points_per_frame=N, loop_ms=1e3 * float(np.median(tl)), add_frames_ms=1e3 * float(np.median(tb)),
               add_frames_device_ms=1e3 * float(np.median(td)))
    out["describe"][K] = row
    print("%5d frames x %d points: loop of mh_place_describe + add %.2f ms, mh_place_db_add_frames from host arrays %.2f ms, from device "
          "arrays %.2f ms; medians of 5 after a warm-up" % (K, N, row["loop_ms"], row["add_frames_ms"], row["add_frames_device_ms"]), flush=True)
    del dev
    for s in scans:
        s.close()

rng = np.random.default_rng(7)
q = rng.integers(0, 256, (20, 64), dtype=np.uint8)
qd = torch.from_numpy(q.reshape(-1)).to("cuda:0")
for K in (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6):
    stored = rng.integers(0, 256, (K, 20 * 64), dtype=np.uint8)
    db = capi.PlaceDB(ctx, cp).add(stored)
    od = torch.zeros((K, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    host_ms = median_ms(lambda: db.search(q))
    dev_ms = median_ms(lambda: db.search_device(qd.data_ptr(), od.data_ptr()))
    got = db.search(q)
    assert np.array_equal(od.cpu().numpy().astype(np.uint32), np.stack([got["shift"], got["dist"]], 1))
    out["search"][K] = dict(descriptors=K, host_out_ms=host_ms, device_out_ms=dev_ms)
    print("%8d descriptors of 20 x 64: mh_place_search %.3f ms with the matches to the host, %.3f ms query and matches on the device"
          % (K, host_ms, dev_ms), flush=True)
    db.close()
print(json.dumps({"place_time": out}))
