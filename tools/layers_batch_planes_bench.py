"""The measurements of profiles/layers_batch_planes.md: multi-layer alignments with a Matcher_Point2Plane pair in lock-step
batches (mh_icp_align_layers_batch_planes) against the same alignments one by one.

  seq   N sequences of the stand-alone driver in one process (molahip-lo-cli with N --seq-dir, a host thread each, one
        AlignBatcher) on the default chain with a Matcher_Point2Plane block added on its point layers (the chain of
        tests/test_gpu_icp_layers_batch_planes.py), the method of tools/multi_seq_bench.py.  Variants alternate, --rounds times:
          batched   this build
          off       this build with MOLA_HIP_BATCH_PLANES=0 (every such alignment on its own beside the batches)
          parent    the command line of another build (--parent-root: a tree of the commit before, built), when given
        Prints every run's steady_scans_per_s, then median (min-max) per variant, and whether all trajectories are equal.
  abi   the C-ABI shape of profiles/layers_planes.md (the small workload: 1000 + 1000 points, k = 2 on the even points and a plane
        pair on the odd ones, against the 20 k-point map), --jobs contexts: host clock around one batch call against the same
        jobs through single calls one after the other (--package-root: the single calls of another build).

    python tools/layers_batch_planes_bench.py seq [--scans 200] [--sequences 8] [--rounds 3] [--parent-root DIR] [--variants batched,off]
    python tools/layers_batch_planes_bench.py abi [--jobs 8] [--reps 20] [--what batch|singles] [--package-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANE_BLOCK = """    - class: mp2p_icp_hip::Matcher_Point2Plane
      params:
        distanceThreshold: 1.0
        planeEigenThreshold: 1e-2
        searchRadius: 2.5
        knn: 10
        minimumPlanePoints: 6
        pointLayerMatches:
          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}
"""
ONE_MATCH = '          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}\n'


def plane_chain_text():
    text = open(os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")).read()
    assert text.count(ONE_MATCH) == 1
    return text.replace(ONE_MATCH, ONE_MATCH + PLANE_BLOCK)


def run_cli(cli, seq, n, pipeline, out, env):
    cmd = [cli, "--pipeline", pipeline, "--out", out, "--time-field", "12"]
    for _ in range(n):
        cmd += ["--seq-dir", seq]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    if r.returncode != 0:
        return {"error": r.stderr[-500:]}
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    per = [l for l in lines if "sequence_dir" in l]
    summ = next((l for l in lines if "sequences" in l), None) or per[0]
    return {"steady_scans_per_s": summ["steady_scans_per_s"], "batches": summ.get("batches"), "jobs_per_batch": summ.get("jobs_per_batch"),
            "scans": sum(p["scans"] for p in per), "good": sum(p["good"] for p in per), "tums": [open(p["tum"]).read() for p in per]}


def seq_main(a):
    sys.path.insert(0, ROOT)
    from mola_lidar_odometry_amd import synth_city
    tmp = tempfile.mkdtemp(prefix="molahip_planes_")
    seq, _ = synth_city.write_kitti_drive(tmp, a.scans, time_channel=True)
    pipeline = os.path.join(tmp, "plane_chain.yaml")
    open(pipeline, "w").write(plane_chain_text())
    cli = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
    variants = [("batched", cli, {}), ("off", cli, {"MOLA_HIP_BATCH_PLANES": "0"})]
    if a.parent_root:
        variants.insert(0, ("parent", os.path.join(os.path.abspath(a.parent_root), "mola_lidar_odometry_amd", "molahip-lo-cli"), {}))
    variants = [v for v in variants if v[0] in a.variants.split(",")]
    runs, first = {v[0]: [] for v in variants}, None
    same = True
    for rnd in range(a.rounds):
        for name, exe, env in variants:
            r = run_cli(exe, seq, a.sequences, pipeline, os.path.join(tmp, "%s_%d.tum" % (name, rnd)), env)
            if "error" in r:
                print(name, rnd, json.dumps(r), flush=True)
                continue
            tums = r.pop("tums")
            first = first or tums[0]
            same = same and all(t == first for t in tums)
            runs[name].append(r["steady_scans_per_s"])
            print(name, rnd, json.dumps(r), flush=True)
    out = {"scans_per_sequence": a.scans, "sequences": a.sequences, "all_trajectories_equal": same}
    for name, v in runs.items():
        if v:
            out[name] = {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
    print(json.dumps({"layers_batch_planes_seq": out}))


def abi_main(a):
    sys.path.insert(0, os.path.abspath(a.package_root))
    from mola_lidar_odometry_amd import capi, synth
    w = synth.workload_small()
    edges, planes = np.ascontiguousarray(w.scan_xyz[0::2]), np.ascontiguousarray(w.scan_xyz[1::2])
    plane = dict(knn=10, minimum_plane_points=6, plane_eigen_threshold=1e-2, search_radius=0.8)
    mi = 40
    thr = np.maximum(0.45, 0.9 - 0.45 * np.arange(mi) / 10.0)
    p = capi.ICPParams(max_iterations=mi, kernel_param=np.full(mi, 0.5), threshold=1.0,
                       gn=capi.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))
    jobs, keep = [], []
    for _ in range(a.jobs):
        ctx = capi.Context(0)
        m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
        keep.append((ctx, m))
        jobs.append([dict(map=m, scan=capi.Scan(ctx, edges), threshold=thr),
                     dict(map=m, scan=capi.Scan(ctx, planes), threshold=0.4, plane=plane)])
    guesses = [w.T_guess] * a.jobs

    def batch():
        return capi.icp_align_layers_batch(jobs, guesses, p, pairings_per_point=[[2, 1]] * a.jobs)

    def singles():
        return [capi.icp_align_layers(j, w.T_guess, p, want_trace=False, pairings_per_point=[2, 1]) for j in jobs]

    fn = batch if a.what == "batch" else singles
    for _ in range(a.warm):
        fn()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    print("%-7s %d jobs: %9.3f ms (%.3f - %.3f, %d repetitions); job 0: %d iterations, %s, %d pairings (%d plane) of %d" % (
        a.what, a.jobs, 1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts), a.reps, r[0]["n_iterations"],
        capi.TERM_NAMES[r[0]["termination_reason"]], r[0]["n_final_pairs"], r[0]["n_final_pairs_pt2pl"], r[0]["potential_pairings"]))
    print("pose %s" % " ".join("%.17g" % v for v in np.asarray(r[0]["T"]).reshape(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("seq", "abi"))
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--sequences", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--variants", default="parent,batched,off")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--what", default="batch", choices=("batch", "singles"))
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    (seq_main if a.mode == "seq" else abi_main)(a)


if __name__ == "__main__":
    main()
