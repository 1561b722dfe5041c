"""Milliseconds per alignment of an rgbd-shaped ICP block (a Matcher_Points_DistanceThreshold with pairingsPerPoint 2 on the edge
layers, a Matcher_Point2Plane with KNN + PCA on the plane layers, one Solver_GaussNewton) through the host layer's ICP::align:

  fused     mh_icp_align_layers_planes over both pairs (one device loop; ICP::fusePlaneMatchers)
  generic   the matcher-by-matcher loop (mh_nn_search_k + mh_nn_search_pt2pl_knn to the host, mh_gn_solve from it, per iteration)

The shape: a workload's scan split into its even points (edge layer, k = 2) and its odd points (plane layer) against the
workload's map, the plane parameters of rgbd.yaml:143-151.  Median of --reps warmed alignments, host clock around synchronised
calls; min - max and the iteration count are printed too.

    python tools/layers_planes_bench.py --workload small|c2 --route fused|generic [--reps N] [--package-root DIR]

--package-root: import the package from another tree (a build of another commit: its generic route).
--search N: instead, N launches of each plane search over the same points -- mh_nn_search_pt2pl_knn (k_match_pl_knn) at the
workload's guess and a planes-only alignment of N iterations with the stall test off (k_match_layers_pl) -- for a kernel trace.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_YAML = """
class_name: mp2p_icp::ICP
params:
  maxIterations: %d
  minAbsStep_trans: 1e-4
  minAbsStep_rot: 5e-5
solvers:
  - class: mp2p_icp::Solver_GaussNewton
    params:
      maxIterations: 2
      robustKernel: 'RobustKernel::GemanMcClure'
      robustKernelParam: 0.5
matchers:
  - class: mp2p_icp::Matcher_Points_DistanceThreshold
    params:
      threshold: 0.9
      thresholdAngularDeg: 0
      pairingsPerPoint: 2
      allowMatchAlreadyMatchedGlobalPoints: true
      pointLayerMatches:
        - {global: "localmap", local: "edges", weight: 1.0}
  - class: mp2p_icp::Matcher_Point2Plane
    params:
      distanceThreshold: 0.40
      planeEigenThreshold: 1e-2
      searchRadius: 0.80
      knn: 10
      minimumPlanePoints: 6
      pointLayerMatches:
        - {global: "localmap", local: "planes", weight: 1.0}
"""


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="small", choices=("small", "c2"))
    ap.add_argument("--route", default="fused", choices=("fused", "generic"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=300)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--search", type=int, default=0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from mola_lidar_odometry_amd import capi, synth
    w = synth.workload_by_name(a.workload)
    edges, planes = np.ascontiguousarray(w.scan_xyz[0::2]), np.ascontiguousarray(w.scan_xyz[1::2])
    if a.search:
        ctx = capi.Context(0)
        m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
        s = capi.Scan(ctx, planes)
        for _ in range(a.search):
            r = capi.nn_search_pt2pl_knn(m, s, w.T_guess, 0.4, 1e-2, 0.8, 10, 6)
        print("k_match_pl_knn: %d launches over %d points, %d pairings at the guess" % (a.search, len(planes), len(r["local_idx"])))
        p = capi.ICPParams(max_iterations=a.search, kernel_param=np.full(a.search, 0.5), threshold=1.0, disable_stall_test=True,
                           gn=capi.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))
        r = capi.icp_align_layers([dict(map=m, scan=s, threshold=0.4, plane=dict(knn=10, minimum_plane_points=6,
                                                                                  plane_eigen_threshold=1e-2, search_radius=0.8))],
                                  w.T_guess, p, want_trace=False)
        print("k_match_layers_pl: %d iterations over %d points, %d final pairings (MH_NO_PREV_BOUND=%s)" % (
            r["n_iterations"], len(planes), r["n_final_pairs"], os.environ.get("MH_NO_PREV_BOUND", "0")))
        return
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip as hl
    icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(_YAML % a.max_iterations))
    icp.fuseMultiPairings(True)
    if a.route == "fused":
        icp.fusePlaneMatchers(True)
    g = hl.metric_map_t()
    hv = hl.HashedVoxelPointCloud(w.voxel_size, w.cap)
    hv.setPoints(w.map_xyz)
    g.set_layer("localmap", hv)
    loc = hl.metric_map_t()
    loc.set_layer("edges", hl.PointCloud(edges))
    loc.set_layer("planes", hl.PointCloud(planes))
    guess = hl.TPose3D(*w.guess_ypr)
    path = icp.alignPath()
    assert path == ("layers" if a.route == "fused" else "generic"), path
    ms, lo, hi, r = timed(lambda: icp.align(loc, g, guess, params), a.reps, a.warm)
    its = r.nIterations + (0 if r.terminationReason.name == "MaxIterations" else 1)
    print("%-7s %-5s %9.3f ms / alignment (%.3f - %.3f, %d repetitions): %d iterations, %s, %d pairings (%d plane) of %d; "
          "%.1f us / ICP iteration; edges %d, planes %d, map %d points" % (
              a.route, a.workload, ms, lo, hi, a.reps, r.nIterations, r.terminationReason.name, r.n_pairs(), r.n_pairs_pt2pl(),
              r.potential_pairings(), 1e3 * ms / max(its, 1), len(edges), len(planes), len(w.map_xyz)))
    print("pose %s" % " ".join("%.9f" % v for v in r.pose()))


if __name__ == "__main__":
    main()
