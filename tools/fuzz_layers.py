"""development aid: random multi-layer alignments (mh_icp_align_layers) against the float64 reference oracle/layers_oracle.py --
1-8 pairs over 1-3 maps (shared maps, shared scans), voxel sizes, caps, floor / trunc indexing, NDT maps, scan sizes on the
workgroup edges of the match (64), accumulation (1024) and covariance (256) grids, empty and one-point scans, NaN / Inf points,
per-pair schedules, angular terms and weights, every robust kernel, 1-4 inner steps, min_delta / max_cost, priors, the device
hook, the stall test, polling, expected_iterations, MH_NO_GRAPH / MH_NO_PREV_BOUND / MH_NO_QIDX.  Exact: iteration count,
termination reason, pairing counts per iteration and per pair, every pair's final local_idx / global_idx / d2, quality; poses
to 1e-7; covariance to the tolerance of the parity suite.  A one-pair case is also bitwise mh_icp_align under MH_MATCH=f, and a
few cases are run again on the warm context at the end: bitwise their first run.  A case whose run decides a stall, hook,
min_delta or max_cost comparison within 1e-9 (relative) of its threshold, or solves normal equations with a condition number
above 1e10 (one or two distinct pairings in all: the step is then made of rounding, on the device as in any float64
restatement), is listed apart with that evidence, and whether it agreed anyway.

fuzz_layers.py [cases [seed [dense]]]: with the third argument `dense` the maps are tests/dense_cases.py's (the uncapped dense-voxel
maps room, mixed and room_clear and the cap-20 map beside them) instead of the outdoor scene, the scans 1 to 2561 points of the
room with points pushed a voxel out of its walls; every other draw, and the default draws, are unchanged."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mola_lidar_odometry_amd import capi, synth  # noqa: E402
from oracle import layers_oracle, oracle_c  # noqa: E402

oracle_c.build()
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 11)
ctx = capi.Context(0)
scene = synth.make_scene(4711, 70.0, 20)
SWITCHES = ("MH_NO_GRAPH", "MH_NO_PREV_BOUND", "MH_NO_QIDX", "MH_MATCH")
for k in SWITCHES:
    os.environ.pop(k, None)


def scan_size():
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return int(rng.choice([0, 1]))
    if kind == 4:
        return int(rng.integers(2, 60000))
    edge = {1: 64, 2: 1024, 3: 256, 5: 1024}[kind]
    return max(0, edge * int(rng.integers(1, 58 if edge == 1024 else 200)) + int(rng.choice([-1, 0, 1])))


dense = len(sys.argv) > 3 and sys.argv[3] == "dense"
if dense:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_cases as dc  # noqa: E402
    dense_inp = dc.Inputs()


def dense_inputs():
    """(pose, cloud, points per map, map arguments, a scan-size draw) from the dense-cell inputs"""
    T_gt = dc.pose(float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.1, 0.2)), float(rng.uniform(-0.2, 0.2)),
                   float(rng.normal(0, 0.01)), float(rng.normal(0, 0.01)))
    cloud = dc.draw_scan(dense_inp.maps["room"][0], T_gt, 4000, rng)
    keys = [str(k) for k in rng.choice(["room", "mixed", "room_clear", "capped"], int(rng.integers(1, 4)))]
    mps = [dense_inp.maps[k][0] for k in keys]
    maps = [(dense_inp.maps[k][1], dense_inp.maps[k][2], 0, dense_inp.maps[k][3]) for k in keys]
    return T_gt, cloud, mps, maps


def make_case():
    if dense:
        T_gt, cloud, mp, maps = dense_inputs()
        n_maps, n_pairs = len(maps), int(rng.integers(1, 5))
        scans = [cloud[rng.choice(len(cloud), int(rng.choice([1, 63, 64, 65, 129, 700, 2000, 2561])), replace=False)].copy()
                 for _ in range(int(rng.integers(1, min(n_pairs, 3) + 1)))]
        iters = int(rng.integers(12, 21))
        thr0, kp = dc.schedule(iters, float(rng.uniform(0.8, 1.5))), np.full(iters, 0.3)
        pairs = [dict(map=int(rng.integers(0, n_maps)), scan=int(rng.integers(0, len(scans))), threshold=float(rng.uniform(0.7, 1.2)) * thr0,
                      threshold_angular_deg=0.0, weight=float(rng.choice([1.0, float(rng.uniform(0.1, 5.0))]))) for _ in range(n_pairs)]
        d = rng.normal(0, 1, 6)
        off = np.concatenate([d[:3] * float(rng.uniform(0.03, 0.15)) / np.linalg.norm(d[:3]), d[3:] * np.deg2rad(0.6)])
        guess = oracle_c.pose_compose(T_gt, dc.pose(*off))
        gkw = dict(max_inner_iterations=int(rng.integers(1, 5)), robust_kernel=int(rng.integers(0, 6)),
                   min_delta=float(rng.choice([0.0, 1e-7, 1e-4])), max_cost=0.0)
        kw = dict(max_iterations=iters, kernel_param=kp, disable_stall_test=bool(rng.integers(0, 2)))
        prior = (T_gt, dc.PRIOR_INFO) if rng.integers(0, 3) == 0 else None
        if sum(len(scans[i]) for i in {e["scan"] for e in pairs}) < 63:  # (one-point layers alone do not hold six dimensions: the
            prior = (T_gt, dc.PRIOR_INFO)                                #  weak prior of the fixed cases, or the case is set apart)
        ctl = dict(poll_every=int(rng.choice([0, 0, 1, 3, 7])), expected_iterations=0)
        sw = [k for k in SWITCHES[:3] if rng.integers(0, 4) == 0]
        return dict(mp=mp, maps=maps, scans=scans, pairs=pairs, guess=guess, gkw=gkw, kw=kw, prior=prior, ctl=ctl, sw=sw)
    pose = [float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), synth.SENSOR_H, float(rng.uniform(-0.2, 0.2)), 0.002, -0.002]
    cloud = synth.make_scan(scene, pose, rings=64, azimuths=1000, seed=int(rng.integers(1, 10000)))
    mp = synth.make_map(scene, int(rng.choice([40000, 100000])), int(rng.integers(1, 10000)))
    n_maps, n_pairs = int(rng.integers(1, 4)), int(rng.integers(1, 9))
    maps = []
    for _ in range(n_maps):
        vs = float(rng.uniform(0.25, 2.0))
        if rng.integers(0, 4) == 0:
            margs = (vs, int(rng.choice([0, 12, 48])), 0, float(rng.choice([0.0, 0.1])), 0.05, 4)  # NDT map
        else:
            margs = (vs, int(rng.choice([0, 1, 3, 20, 48])), int(rng.integers(0, 2)))
        maps.append(margs)
    scans = []
    for _ in range(int(rng.integers(1, min(n_pairs, 4) + 1))):
        n = scan_size()
        s = cloud[rng.choice(len(cloud), n, replace=n > len(cloud))].copy()
        if n > 4 and rng.integers(0, 4) == 0:
            bad = rng.choice(n, min(n, int(rng.integers(1, 20))), replace=False)
            s[bad, int(rng.integers(0, 3))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
        scans.append(s)
    iters = int(rng.integers(1, 61))
    thr0, kp = synth.threshold_schedule(float(rng.choice([0.5, 1.0, 2.0])), iters)
    pairs = []
    for i in range(n_pairs):
        f = float(rng.uniform(0.3, 0.6)) if (i == 0 and rng.integers(0, 3) == 0) else float(rng.uniform(0.6, 2.0))
        w = float(rng.choice([1.0, float(rng.uniform(0.0, 5.0)), 0.0], p=[0.4, 0.4, 0.2]))
        pairs.append(dict(map=int(rng.integers(0, n_maps)), scan=int(rng.integers(0, len(scans))), threshold=f * thr0,
                          threshold_angular_deg=float(rng.choice([0.0, float(rng.uniform(0.0, 1.0))])), weight=w))
    d = rng.normal(0, 1, 3)
    d *= float(rng.uniform(0.02, 0.6)) / np.linalg.norm(d)
    guess = synth.pose_from_ypr(np.array(pose) + [d[0], d[1], 0.1 * d[2], float(rng.normal(0, 0.01)), 0.002, 0.001])
    gkw = dict(max_inner_iterations=int(rng.integers(1, 5)), robust_kernel=int(rng.integers(0, 6)),
               min_delta=float(rng.choice([0.0, 1e-7, 1e-4])), max_cost=float(rng.choice([0.0, 0.0, 1e-3])))
    kw = dict(max_iterations=iters, kernel_param=kp, disable_stall_test=bool(rng.integers(0, 3) == 0),
              min_abs_step_trans=float(rng.choice([1e-4, 5e-4])), min_abs_step_rot=float(rng.choice([5e-5, 1e-4, 5e-4])))
    if rng.integers(0, 4) == 0:
        kw.update(hook_enabled=True, hook_min_trans=float(rng.choice([0.05, 0.2])), hook_min_rot=float(np.deg2rad(0.75)))
    prior = None
    if rng.integers(0, 4) == 0:
        prior = (guess, np.diag([20.0, 20.0, 20.0, 300.0, 300.0, 300.0]) * float(rng.choice([0.1, 1.0, 10.0])))
    ctl = dict(poll_every=int(rng.choice([0, 0, 1, 3, 7, 64])), expected_iterations=int(rng.choice([0, 0, int(rng.integers(1, 61))])))
    sw = [k for k in SWITCHES[:3] if rng.integers(0, 4) == 0]
    return dict(mp=mp, maps=maps, scans=scans, pairs=pairs, guess=guess, gkw=gkw, kw=kw, prior=prior, ctl=ctl, sw=sw)


def run_device(c, g_maps, g_scans, match=None):
    for k in SWITCHES:
        os.environ.pop(k, None)
    for k in c["sw"]:
        os.environ[k] = "1"
    if match:
        os.environ["MH_MATCH"] = match
    try:
        p = capi.ICPParams(gn=capi.GNParams(**c["gkw"]), **c["kw"], **c["ctl"])
        return capi.icp_align_layers([dict(map=g_maps[e["map"]], scan=g_scans[e["scan"]], threshold=e["threshold"],
                                           threshold_angular_deg=e["threshold_angular_deg"], weight=e["weight"]) for e in c["pairs"]],
                                     c["guess"], p, prior=c["prior"], want_pairs=True)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def run_single(c, g_maps, g_scans):
    """The one pair as mh_icp_align with MH_MATCH=f."""
    e = c["pairs"][0]
    os.environ["MH_MATCH"] = "f"
    for k in c["sw"]:
        os.environ[k] = "1"
    try:
        p = capi.ICPParams(gn=capi.GNParams(weight_pt2pt=e["weight"], **c["gkw"]), threshold=e["threshold"],
                           threshold_angular_deg=e["threshold_angular_deg"], **c["kw"], **c["ctl"])
        return capi.icp_align(g_maps[e["map"]], g_scans[e["scan"]], c["guess"], p, prior=c["prior"], want_pairs=True)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def bitwise(a, b, single=False):
    same = (np.array_equal(a["T"], b["T"]) and np.array_equal(a["cov"], b["cov"]) and
            all(a[k] == b[k] for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "quality")) and
            [t["n_pairs"] for t in a["trace"]] == [t["n_pairs"] for t in b["trace"]] and
            all(np.array_equal(x["T"], y["T"]) for x, y in zip(a["trace"], b["trace"])))
    pa = a["pairs"] if not single else [a["pairs"]]
    pb = b["pairs"] if not single else [b["pairs"]]
    return same and all(np.array_equal(x[k], y[k]) for x, y in zip(pa, pb) for k in ("local_idx", "global_idx", "d2"))


bad, near, kept = 0, [], []
for case in range(n_cases):
    c = make_case()
    mps = c["mp"] if isinstance(c["mp"], list) else [c["mp"]] * len(c["maps"])  # (dense: every map its own points)
    g_maps = [capi.Map(ctx, *m).build(q) for m, q in zip(c["maps"], mps)]
    o_maps = [oracle_c.Map(*m).insert(q) for m, q in zip(c["maps"], mps)]
    g_scans = [capi.Scan(ctx, s) for s in c["scans"]]
    try:
        r = run_device(c, g_maps, g_scans)
        op = oracle_c.ICPParams(gn=oracle_c.GNParams(**c["gkw"]), **c["kw"])
        o = layers_oracle.icp_align_layers([dict(map=o_maps[e["map"]], local=c["scans"][e["scan"]], threshold=e["threshold"],
                                                 threshold_angular_deg=e["threshold_angular_deg"], weight=e["weight"])
                                            for e in c["pairs"]], c["guess"], op, prior=c["prior"], n_threads=16)
        diffs = layers_oracle.compare(r, o)
        same_single = True  # device against device: never set apart
        if len(c["pairs"]) == 1:
            s = run_single(c, g_maps, g_scans)
            same_single = bitwise(dict(r, pairs=r["pairs"][0]), s, single=True) and r["pair_counts"] == [s["n_final_pairs"]]
        nd = layers_oracle.nearest_decision(o["margins"])
        ok = not diffs
        if nd is not None and nd[1] <= 1e-9:
            near.append((case, "%s decided %.2e (relative) from its threshold" % nd, diffs))
            ok = True  # reported apart below, with its evidence
        elif o["max_cond"] > 1e10:
            near.append((case, "normal equations of condition number %.1e (%d pairings in the first iteration)" % (
                o["max_cond"], r["trace"][0]["n_pairs"] if r["trace"] else r["n_final_pairs"]), diffs))
            ok = True
        if ok and len(kept) < 4 and case % 3 == 0:
            kept.append((case, c, g_maps, g_scans, r))
        if not same_single:
            ok = False
            diffs.append("one pair differs from mh_icp_align (MH_MATCH=f)")
        note = "iters %d term %s pairs %s" % (r["n_iterations"], capi.TERM_NAMES[r["termination_reason"]], r["pair_counts"])
        if diffs:
            note += " | " + "; ".join(diffs)
    except capi.MolahipError as e:
        ok, note = False, "ERROR " + str(e)[-120:]
    bad += 0 if ok else 1
    print("case %3d pairs=%d maps=%s scans=%s inner=%d kernel=%d min_delta=%g max_cost=%g stall_off=%d hook=%d prior=%d "
          "poll=%d expect=%d sw=%s %s -> %s" % (
              case, len(c["pairs"]), [("ndt" if len(m) > 4 else "trunc" if m[2] else "floor", round(m[0], 2), m[1]) for m in c["maps"]],
              [len(s) for s in c["scans"]], c["gkw"]["max_inner_iterations"], c["gkw"]["robust_kernel"], c["gkw"]["min_delta"],
              c["gkw"]["max_cost"], c["kw"]["disable_stall_test"], "hook_enabled" in c["kw"], c["prior"] is not None,
              c["ctl"]["poll_every"], c["ctl"]["expected_iterations"], ",".join(s[3:] for s in c["sw"]) or "-", note,
              "ok" if ok else "MISMATCH"), flush=True)
for case, c, g_maps, g_scans, r in kept:  # the same inputs on the now warm context: bitwise the first run
    again = run_device(c, g_maps, g_scans)
    same = bitwise(again, r) and again["pair_counts"] == r["pair_counts"]
    bad += 0 if same else 1
    print("rerun of case %d on the warm context: %s" % (case, "bitwise equal" if same else "MISMATCH"), flush=True)
for case, why, diffs in near:
    print("case %d apart: %s; %s" % (case, why, "; ".join(diffs) if diffs else "agrees with the reference anyway"))
print("cases apart (near a threshold or ill-conditioned):", len(near))
print("mismatches:", bad)
sys.exit(1 if bad else 0)
