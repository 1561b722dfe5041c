"""Measurements of profiles/rgbd.md on the GPU:  python tools/rgbd_measure.py [out.json]
Time per call of mh_scan_edges_from_range_image at 160 x 120 and 640 x 480 (host clock around calls that end in a stream wait, 30
calls of warm-up, 5 x 200 timed) from device, page-locked and pageable memory; the 30-frame test drive (tests/rgbd_inline.py)
with localmap_planes as SparseTreesPointCloud and as HashedVoxelPointCloud (the same cell, cap 20): frames/s, host time of
an alignment, and of a key-frame insertion including the wait for it."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from mola_lidar_odometry_amd import capi
from mola_lidar_odometry_amd import _mp2p_icp_hip as H
import rgbd_inline as RG
import rimg_ref as RR

out = {}
ctx = capi.Context(0)
for rows, cols in ((120, 160), (480, 640)):
    # the test room at either size (the same camera, scaled)
    s = cols / RG.COLS
    RG.ROWS, RG.COLS, RG.FX, RG.FY, RG.CX, RG.CY = rows, cols, 140.0 * s, 140.0 * s, (cols - 1) / 2, (rows - 1) / 2
    img = RG.render(np.eye(4))
    p = capi.range_image_params(rows, cols, RG.FX, RG.FY, RG.CX, RG.CY, RG.RANGE_UNITS, True, RG.SENSOR_POSE)
    e, q = capi.Scan(ctx), capi.Scan(ctx)
    dev = torch.from_numpy(img.view(np.int16).copy()).cuda(); torch.cuda.synchronize()
    pin = torch.from_numpy(img.view(np.int16).copy()).pin_memory()
    res = {}
    for name, src, mem in (("device", dev.data_ptr(), capi.MEM_DEVICE), ("pinned", pin.data_ptr(), capi.MEM_HOST_PINNED),
                           ("host", img, capi.MEM_HOST)):
        for _ in range(30):
            capi.scan_edges_from_range_image(ctx, src, p, e, q, mem)
        reps = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(200):
                capi.scan_edges_from_range_image(ctx, src, p, e, q, mem)  # (the call ends in a stream wait)
            reps.append((time.perf_counter() - t0) / 200 * 1e6)
        res[name + "_us_per_call"] = [round(v, 1) for v in reps]
    ne, nq = len(e), len(q)
    res.update(n_edges=ne, n_planes=nq, bytes_read=2 * rows * cols, bytes_words=2 * 8 * rows * cols * 2,
               bytes_points=16 * (ne + nq))
    out[f"generator_{cols}x{rows}"] = res
    print(cols, rows, res, flush=True)
RG.ROWS, RG.COLS, RG.FX, RG.FY, RG.CX, RG.CY = 120, 160, 140.0, 140.0, 79.5, 59.5

drv = RG.drive(30)
def drive(text):
    lo = H.LidarOdometry(0, True)
    lo.initialize(H.Config.FromYamlText(text))
    ins = []
    t0 = time.perf_counter()
    for st, img in zip(drv[0], drv[2]):
        rec = lo.onDepthImage(float(st), img, **RG.CAMERA)
        if rec["map_updated"]:
            a = time.perf_counter(); lo.localMapSizes(); ins.append(time.perf_counter() - a)  # wait for the insertion
    dt = time.perf_counter() - t0
    pr = lo.profile(); recs = lo.records()
    n_al = sum(r["align_calls"] for r in recs)
    return dict(frames_per_s=round(30 / dt, 1), align_ms=round(1e3 * pr["onLidar.3.run_icp"] / n_al, 3), alignments=n_al,
                iterations=int(pr["icp.executed_iterations"]),
                insert_ms=round(1e3 * (pr["onLidar.4.update_local_map"] + sum(ins)) / len(ins), 3), inserts=len(ins),
                generator_ms=round(1e3 * pr["onLidar.0.upload_raw"] / 30, 3), filter_1st_ms=round(1e3 * pr["onLidar.1.filter_1st"] / 30, 3),
                maps=lo.localMapStats())
for name, text in (("sparse_trees", RG.pipeline()), ("hashed_cap20", RG.pipeline(RG.HASHED_PLANES.format(cap=20)))):
    drive(text)  # warm-up: code objects, graphs
    out[name] = [drive(text) for _ in range(3)]
    for r in out[name]: print(name, r, flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=str)
