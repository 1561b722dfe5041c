"""development aid: random alignments (voxel size, cap, index mode, guess error, layer size, matcher) against the CPU oracle --
per-iteration pair counts, final pairings and d2 bit for bit, poses to 1e-9.  Exercises the previous-pairing bound and its
fallback (large guess errors with small voxels) beyond the fixed cases of tests/test_gpu_parity.py.

fuzz_bound.py [cases [seed [dense]]]: with the third argument `dense` the maps are tests/dense_cases.py's uncapped dense-voxel maps
(room, mixed, room_clear) instead of the outdoor scene, the layers 1 to 2561 points of them with points pushed a voxel out of the
walls, the guess 3 to 15 cm and about a degree off; the default draws are unchanged."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mola_lidar_odometry_amd import capi, synth  # noqa: E402
from oracle import oracle_c  # noqa: E402

oracle_c.build()
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
ctx = capi.Context(0)
bad = 0
dense = len(sys.argv) > 3 and sys.argv[3] == "dense"
if dense:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_cases as dc  # noqa: E402
    inp = dc.Inputs()
for case in range(n_cases if dense else 0):
    mk = str(rng.choice(["room", "mixed", "room_clear"]))
    pts, vs, cap, md = inp.maps[mk]
    n_scan = int(rng.choice([1, 63, 64, 65, 129, 700, 2000, 2561]))
    match = str(rng.choice(["f", "q", "s", "p", "x", "f", "s"]))
    T_gt = dc.pose(float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.1, 0.2)), float(rng.uniform(-0.2, 0.2)),
                   float(rng.normal(0, 0.01)), float(rng.normal(0, 0.01)))
    scan = dc.draw_scan(pts, T_gt, n_scan, rng)
    d = rng.normal(0, 1, 6)
    off = np.concatenate([d[:3] * float(rng.uniform(0.03, 0.15)) / np.linalg.norm(d[:3]), d[3:] * np.deg2rad(0.6)])
    guess = oracle_c.pose_compose(T_gt, dc.pose(*off))
    iters = int(rng.choice([12, 16, 20]))
    kw = dict(max_iterations=iters, threshold=dc.schedule(iters, float(rng.uniform(0.8, 1.5))), kernel_param=np.full(iters, 0.3),
              disable_stall_test=bool(rng.integers(0, 2)))
    prior = None
    if n_scan < 700:  # (a small layer does not hold six dimensions: the weak prior of the fixed cases)
        prior = (T_gt, dc.PRIOR_INFO)
    sw = [k for k in ("MH_NO_PREV_BOUND", "MH_NO_QIDX", "MH_NO_GRAPH") if rng.integers(0, 4) == 0]
    o = oracle_c.icp_align(oracle_c.Map(vs, cap, 0, md).insert(pts), scan, guess, oracle_c.ICPParams(**kw), prior=prior, want_pairs=True)
    os.environ["MH_MATCH"] = match
    for k in sw:
        os.environ[k] = "1"
    g = capi.icp_align(capi.Map(ctx, vs, cap, 0, md).build(pts), capi.Scan(ctx, scan), guess, capi.ICPParams(**kw), prior=prior,
                       want_pairs=True)
    for k in sw:
        del os.environ[k]
    ok = (g["n_iterations"] == o["n_iterations"] and g["termination_reason"] == o["termination_reason"] and
          [t["n_pairs"] for t in g["trace"]] == [t["n_pairs"] for t in o["trace"]] and
          all(np.array_equal(g["pairs"][k], o["pairs"][k]) for k in ("local_idx", "global_idx", "d2", "global_xyz")) and
          float(np.abs(g["T"] - o["T"]).max()) < 1e-9)
    bad += 0 if ok else 1
    print("case %2d dense map=%-10s n=%4d match=%s sw=%s iters=%d pairs=%d -> %s" % (
        case, mk, n_scan, match, ",".join(k[3:] for k in sw) or "-", g["n_iterations"], g["n_final_pairs"], "ok" if ok else "MISMATCH"),
        flush=True)
for case in range(0 if dense else n_cases):
    vs = float(rng.choice([0.2, 0.35, 0.5, 1.0, 1.7]))
    cap = int(rng.choice([0, 3, 8, 20, 40]))
    mode = int(rng.choice([0, 0, 1]))
    n_scan = int(rng.choice([1500, 4000, 9000, 20000, 24000]))
    shift = float(rng.uniform(0.05, 1.2))
    # f: the plan / scan matcher (default of large layers, round 5); ten entries, so that a seed keeps drawing the cases it always drew
    match = str(rng.choice(["f", "q", "s", "f", "s", "f", "f", "f", "p", "f"]))
    seed = int(rng.integers(1, 10000))
    scene = synth.make_scene(seed, 60.0, 20)
    mp = synth.make_map(scene, int(rng.choice([40000, 150000])), seed)
    pose = [float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), synth.SENSOR_H, float(rng.uniform(-0.2, 0.2)), 0.002, -0.002]
    scan = synth.make_scan(scene, pose, rings=48, azimuths=500, seed=seed + 1)[:n_scan]
    d = rng.normal(0, 1, 3)
    d *= shift / np.linalg.norm(d)
    guess = synth.pose_from_ypr(np.array(pose) + [d[0], d[1], 0.1 * d[2], float(rng.normal(0, 0.02)), 0.003, 0.002])
    iters = int(rng.choice([15, 40]))
    thr, kp = synth.threshold_schedule(2.0, iters)
    kw = dict(max_iterations=iters, threshold=thr, kernel_param=kp)
    if rng.integers(0, 3) == 0:  # converge all the way: the inner Gauss-Newton loop then ends early (step < min_delta)
        iters = 60
        thr, kp = synth.threshold_schedule(2.0, iters)
        kw = dict(max_iterations=iters, threshold=thr, kernel_param=kp, disable_stall_test=True)
    o = oracle_c.icp_align(oracle_c.Map(vs, cap, mode).insert(mp), scan, guess, oracle_c.ICPParams(**kw), want_pairs=True)
    os.environ["MH_MATCH"] = match
    g = capi.icp_align(capi.Map(ctx, vs, cap, mode).build(mp), capi.Scan(ctx, scan), guess, capi.ICPParams(**kw), want_pairs=True)
    ok = (g["n_iterations"] == o["n_iterations"] and g["termination_reason"] == o["termination_reason"] and
          [t["n_pairs"] for t in g["trace"]] == [t["n_pairs"] for t in o["trace"]] and
          all(np.array_equal(g["pairs"][k], o["pairs"][k]) for k in ("local_idx", "global_idx", "d2", "global_xyz")) and
          float(np.abs(g["T"] - o["T"]).max()) < 1e-9)
    bad += 0 if ok else 1
    print("case %2d vs=%.2f cap=%2d mode=%d n=%5d shift=%.2f match=%s iters=%d pairs=%d -> %s" % (
        case, vs, cap, mode, n_scan, shift, match, g["n_iterations"], g["n_final_pairs"], "ok" if ok else "MISMATCH"), flush=True)
print("mismatches:", bad)
sys.exit(1 if bad else 0)
