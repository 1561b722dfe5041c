"""Measurements of profiles/radius_search.md on the GPU:  python tools/radius_measure.py [out.json] [--calls N]
mh_nn_search_radius on the C2 shapes (120 k-point scan against the 1 M-point map, voxel 1.0, cap 20) at r = 0.5 and r = 1.0, both
flags: host-clock medians of repeated blocking calls after a warm-up -- the count-only call, the sized call into device arrays and
the sized call into host arrays -- plus mh_nn_search_k (k = 8, threshold r) on the same inputs as a yardstick, and the bytes the
fill pass has to move.  The split into count / scan / fill / sort + gather comes from a kernel trace of this script run with
--calls 3 (rocprofv3 --kernel-trace --stats): the library has no timers of its own."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mola_lidar_odometry_amd import capi, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 30
warm = min(5, calls)

w = synth.workload_c2()
ctx = capi.Context(0)
m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
s = capi.Scan(ctx, w.scan_xyz)
T = np.ascontiguousarray(np.asarray(w.T_guess, np.float64).reshape(-1)[:12])
Tp = T.ctypes.data_as(C.POINTER(C.c_double))
L = capi.lib()
n = s.n
out = dict(scan_points=n, map_points=int(m.info().n_points), voxel_size=w.voxel_size, cap=w.cap, calls=calls, warm_up=warm)


def median_ms(f):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()  # (blocking: every call ends in a stream wait)
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)


def ptr(t):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_uint32 if t.dtype == torch.int32 else C.c_float))


for radius in (0.5, 1.0):
    for flags, name in ((capi.RADIUS_VISIT_ORDER, "visit"), (capi.RADIUS_SORTED, "sorted")):
        info = capi.RadiusInfo()
        count_only = lambda: capi._chk(L.mh_nn_search_radius(m._h, s._h, Tp, radius, flags, None, capi.MEM_HOST, C.byref(info)))  # noqa: E731
        count_only()
        k = int(info.n_results)
        dev = torch.device("cuda:0")
        d_off, d_gi = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.int32, device=dev)
        d_f = [torch.zeros(k, dtype=torch.float32, device=dev) for _ in range(4)]
        torch.cuda.synchronize()
        o_dev = capi.RadiusOut(ptr(d_off), ptr(d_gi), *[ptr(a) for a in d_f], k)
        h_off, h_gi, h_f = np.zeros(n + 1, np.uint32), np.zeros(k, np.uint32), [np.zeros(k, np.float32) for _ in range(4)]
        o_host = capi.RadiusOut(h_off.ctypes.data_as(C.POINTER(C.c_uint32)), h_gi.ctypes.data_as(C.POINTER(C.c_uint32)),
                                *[a.ctypes.data_as(C.POINTER(C.c_float)) for a in h_f], k)
        sized_dev = lambda: capi._chk(L.mh_nn_search_radius(m._h, s._h, Tp, radius, flags, C.byref(o_dev), capi.MEM_DEVICE, C.byref(info)))  # noqa: E731
        sized_host = lambda: capi._chk(L.mh_nn_search_radius(m._h, s._h, Tp, radius, flags, C.byref(o_host), capi.MEM_HOST, C.byref(info)))  # noqa: E731
        r = dict(n_results=k, max_per_query=int(info.max_per_query), results_per_point=round(k / n, 2),
                 # what the fill pass must move: a 16-byte record read per hit, five 4-byte result entries written (sorted: an
                 # 8-byte key more, then key + index through the sort and 20 bytes read + 20 written by the gather)
                 fill_bytes_min=k * (16 + 20) + (k * (8 + 2 * 12 + 40) if flags else 0),
                 count_only_ms=median_ms(count_only), sized_device_ms=median_ms(sized_dev), sized_host_ms=median_ms(sized_host))
        assert int(info.n_written) == k and h_off[-1] == k and (d_off.cpu().numpy().view(np.uint32) == h_off).all()
        out[f"r{radius}_{name}"] = r
        print(radius, name, r, flush=True)
    out[f"r{radius}_nn_search_k8_host_ms"] = median_ms(lambda: capi.nn_search_k(m, s, T, radius, 8))
    print(radius, "nn_search_k k=8", out[f"r{radius}_nn_search_k8_host_ms"], flush=True)

if args:
    json.dump(out, open(args[0], "w"), indent=1)
