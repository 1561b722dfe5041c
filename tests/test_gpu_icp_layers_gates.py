"""Matcher::runFromIteration / runUpToIteration per pair on the fused multi-layer loop (mh_icp_align_layers_gated): a pair outside
its interval neither searches nor contributes -- no pairings, no claims, nothing in the covariance, the final pairings, the counts.

Checked against the float64 reference oracle/layers_oracle.py with the gate (and the serial claim walk) as its matcher
(tests/gates_ref.py, which also holds the inputs: tests/test_gates_cpu.py shows on the CPU that none of them decides anything
within rounding and that the gates change every result), at layers_oracle.compare's own bars; against exact identities (stale
pairing buffers, all gates 0, graph replay, polling); through the host layer against its matcher-by-matcher loop; and through the
stand-alone driver on the reference's lidar3d-near-far.yaml.

The parent of this change has neither the entry point nor the setter, so every test here fails there at the binding.  A library
that took the call and ignored the gates would compute the ungated alignments, and tests/test_gates_cpu.py shows on the reference
that those differ from the gated ones in every case of 1-7 (pairing counts of the gated iterations, which are compared exactly)."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest

import gates_ref as G
from mola_lidar_odometry_amd import capi, synth
from oracle import layers_oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
REF_NEAR_FAR = "/root/reference/pipelines/extras/lidar3d-near-far.yaml"


class _World:
    """The inputs of gates_ref on one context: device maps, the reference's maps, and every case's reference (computed once)."""

    def __init__(self, inp, ctx=None):
        self.inp = inp
        self.ctx = ctx if ctx is not None else capi.Context(0)
        self.maps = {k: capi.Map(self.ctx, vs, cap).build(pts) for k, (pts, vs, cap) in inp.maps.items()}

    def pairs(self, c, gated=True, locals_=None, shift=0):
        """`shift`: pair i on the map of pair i + shift (the stale-buffer runs: records of another map in every segment)"""
        n = len(c["pairs"])
        return [dict(map=self.maps[c["pairs"][(i + shift) % n]["map"]], scan=capi.Scan(self.ctx, e["local"] if locals_ is None else locals_[i]),
                     threshold=e["threshold"], threshold_angular_deg=e["threshold_angular_deg"], weight=e["weight"],
                     unique_global=e["unique"], run_from_iteration=e["gate"][0] if gated else 0,
                     run_up_to_iteration=e["gate"][1] if gated else 0) for i, e in enumerate(c["pairs"])]


def _params(c, **kw):
    p = capi.ICPParams(max_iterations=c["max_it"], kernel_param=c["kp"], threshold=1.0,
                       gn=capi.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4), **c["pkw"], **kw)
    if c["hook"] is not None:
        chk, tr, rot = c["hook"]
        p = replace(p, hook_enabled=True, hook_min_trans=tr, hook_min_rot=rot, hook_checkpoint=chk)
    return p


@pytest.fixture(scope="module")
def inp(small_workload):
    return G.Inputs(small_workload)


@pytest.fixture(scope="module")
def world(inp):
    return _World(inp)


@pytest.fixture(scope="module")
def cases(inp):
    return G.cases(inp)


@pytest.fixture(scope="module")
def refs(oracle, inp, cases):
    """name -> reference, computed on first use and never changed"""
    omaps, cache = inp.omaps(), {}

    def get(name):
        if name not in cache:
            cache[name] = G.case_reference(cases[name], omaps, inp.T0)
        return cache[name]
    return get


def _run(world, c, T0=None, **kw):
    return capi.icp_align_layers(world.pairs(c), world.inp.T0 if T0 is None else T0, _params(c), prior=c["prior"], want_pairs=True, **kw)


def _check(r, o):
    diffs = layers_oracle.compare(r, o)
    assert not diffs, diffs


def _bitwise(a, b):
    for k in ("T", "cov"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "quality", "pair_counts"):
        assert a[k] == b[k], k
    if "trace" in a and "trace" in b:
        assert len(a["trace"]) == len(b["trace"])
        for x, y in zip(a["trace"], b["trace"]):
            assert x["n_pairs"] == y["n_pairs"] and x["threshold"] == y["threshold"]
            np.testing.assert_array_equal(x["T"], y["T"])
    if "pairs" in a and "pairs" in b:
        for x, y in zip(a["pairs"], b["pairs"]):
            for k in ("local_idx", "global_idx", "d2"):
                np.testing.assert_array_equal(x[k], y[k])


def _gates_of(pairs):
    g = (capi.LayerPairGates * len(pairs))()
    for i, e in enumerate(pairs):
        g[i].run_from_iteration, g[i].run_up_to_iteration = e["run_from_iteration"], e["run_up_to_iteration"]
    return g


def _align_gated_raw(pairs, T_guess, p, gates, fill=0):
    """mh_icp_align_layers_gated with `gates` handed over as they are (None: NULL), opts NULL: result, trace and pairs, and the
    struct's bytes.  `fill`: what the pairing buffers hold before the call; they come back whole as `pair_buffers`."""
    cp, keep = replace(p, threshold=1.0).c(T_guess)
    T0 = np.ascontiguousarray(np.asarray(T_guess, np.float64).reshape(-1)[:12])
    arr, norm, thr_keep = capi._layer_pairs(pairs, p.max_iterations)
    n = len(norm)
    res = capi.ICPResult()
    trace = (capi.ICPIter * max(1, p.max_iterations))()
    counts = (C.c_uint64 * n)()
    po, bufs = (capi.PairsOut * n)(), []
    for i, e in enumerate(norm):
        m = max(e["scan"].n, 1)
        li, gi = np.full(m, fill, np.uint32), np.full(m, fill, np.uint32)
        f = [np.full(m, fill, np.float32) for _ in range(4)]
        po[i] = capi.PairsOut(li.ctypes.data_as(capi._UP), gi.ctypes.data_as(capi._UP), *[a.ctypes.data_as(capi._FP) for a in f])
        bufs.append((li, gi, *f))
    st = capi.lib().mh_icp_align_layers_gated(n, arr, None, gates, C.byref(cp), T0.ctypes.data_as(capi._DP), None, C.byref(res), trace,
                                              po, counts, capi.MEM_HOST)
    assert st == 0, st
    out = capi._result_dict(res)
    out["pair_counts"] = [int(v) for v in counts]
    out["trace"] = capi._trace_list(out, trace, p)
    out["pairs"] = [dict(local_idx=b[0][:k].copy(), global_idx=b[1][:k].copy(), d2=b[5][:k].copy())
                    for b, k in zip(bufs, out["pair_counts"])]
    out["pair_buffers"] = bufs
    return out, bytes(res)


# ------------------------------------------------------------------------------------------------------ 1. the near-far shape
@pytest.mark.parametrize("n", G.SIZES)
def test_near_far_shape_with_a_late_pair(world, cases, refs, n):
    """Pair 0 enters at iteration 4 (its first search unbounded, whatever its segment held); pairs 1 and 2 share a scan, pair 2 is
    on pair 0's map.  The gated layer on every edge of the kernels' ranges."""
    c, o = cases["near_far_%d" % n], refs("near_far_%d" % n)
    r = _run(world, c)
    print("n %d: n_pairs per iteration %s, final counts %s" % (n, [t["n_pairs"] for t in r["trace"]], r["pair_counts"]))
    assert o["n_final_pairs"] > 0 and o["pair_counts"][0] > 0
    _check(r, o)
    assert r["potential_pairings"] == n + 2 * len(world.inp.near_l)
    assert r["trace"][0]["threshold"] == c["pairs"][0]["threshold"][0]  # pair 0's schedule, active or not


# ----------------------------------------------------------------------------------------- 2. up_to below the final iteration
def test_a_pair_that_has_left_leaves_nothing_behind(world, cases, refs):
    c, o = cases["up_to"], refs("up_to")
    pairs = world.pairs(c)
    r, _ = _align_gated_raw(pairs, world.inp.T0, _params(c), _gates_of(pairs), fill=SENTINEL)
    assert o["n_iterations"] > 3 + 1
    _check(r, o)  # (the covariance: the reference's, over pair 1's pairings alone)
    assert r["pair_counts"][0] == 0 and r["pair_counts"][1] > 0
    assert r["potential_pairings"] == len(c["pairs"][1]["local"])
    li, gi, gx, gy, gz, d2 = r["pair_buffers"][0]
    assert np.all(li == SENTINEL) and np.all(gi == SENTINEL)
    want = np.full(1, SENTINEL, np.float32)[0]
    for a in (gx, gy, gz, d2):
        assert np.all(a == want)


# --------------------------------------------------------------------------------- 3. from above every executed iteration
def test_a_pair_that_never_runs(world, cases, refs):
    c, o = cases["never"], refs("never")
    r = _run(world, c)
    _check(r, o)
    assert r["pair_counts"][1] == 0
    assert r["potential_pairings"] == 2 * len(world.inp.near_l)


# ------------------------------------------------------------------------------------------------------ 4. from == up_to == k
def test_a_pair_active_for_one_iteration(world, cases, refs):
    c, o = cases["single_iteration"], refs("single_iteration")
    r = _run(world, c)
    tr = [t["n_pairs"] for t in r["trace"]]
    assert tr[2] > tr[1] and tr[3] < tr[2]
    _check(r, o)
    assert r["pair_counts"][0] == 0


# ------------------------------------------------------------------------------------------------------------ 5. stale buffers
@pytest.mark.parametrize("name", ["near_far_1025", "near_far_65", "up_to"])
def test_foreign_pairings_in_the_segments_change_nothing(inp, cases, name):
    """A context whose pairing segments hold another alignment's pairings (the same layout: scans permuted, maps rotated among
    the pairs, another guess, no gates) gives the bits of a fresh context."""
    c = cases[name]
    fresh = _World(inp)
    want = _run(fresh, c)
    used = _World(inp)
    gen = np.random.default_rng(5)
    permuted = [np.ascontiguousarray(e["local"][gen.permutation(len(e["local"]))]) for e in c["pairs"]]
    other = capi.icp_align_layers(used.pairs(c, gated=False, locals_=permuted, shift=1), inp.T1, _params(c))
    assert other["n_final_pairs"] > 0 and all(k > 0 for k in other["pair_counts"])
    got = _run(used, c)
    _bitwise(got, want)


# ------------------------------------------------------------------------------------------------------------- 6. NoPairings
def test_everybody_gated_off_in_iteration_0_is_no_pairings(world, cases, refs):
    c, o = cases["nobody_at_0"], refs("nobody_at_0")
    r = _run(world, c)
    assert capi.TERM_NAMES[o["termination_reason"]] == "NoPairings" and o["n_iterations"] == 0
    _check(r, o)
    assert r["potential_pairings"] == 0 and r["quality"] == 0.0
    np.testing.assert_array_equal(r["T"], world.inp.T0)


def test_an_empty_active_set_in_a_later_iteration_is_no_pairings(world, cases, refs):
    c, o = cases["nobody_at_3"], refs("nobody_at_3")
    r = _run(world, c)
    assert capi.TERM_NAMES[o["termination_reason"]] == "NoPairings" and o["n_iterations"] == 3
    _check(r, o)
    assert r["potential_pairings"] == 0 and r["pair_counts"] == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. gates with unique_global
def test_a_gated_unique_pair_claims_from_its_first_iteration_on(world, cases, refs):
    """Two unique pairs on one map, the first from = 3: until then the second pair keeps map points that the first takes from it
    afterwards -- read from the reference alone before the device is asked."""
    c, o = cases["unique"], refs("unique")
    stolen = 0
    for k1 in range(3, o["n_iterations"]):
        cand_l, cand_g = o["candidates"][(1, k1)]
        kept_l = o["kept"][(1, k1)][0]
        first_g = o["kept"][(0, k1)][1]
        lost = ~np.isin(cand_l, kept_l) & np.isin(cand_g, first_g)   # dropped at k1, its map point held by pair 0
        for k0 in range(3):
            l0, g0 = o["kept"][(1, k0)]
            had = dict(zip(l0.tolist(), g0.tolist()))
            stolen += sum(1 for l, g in zip(cand_l[lost].tolist(), cand_g[lost].tolist()) if had.get(l) == g)
    print("pairings pair 1 kept before iteration 3 and lost to pair 0 afterwards: %d" % stolen)
    assert stolen >= 1
    assert all(len(o["kept"][(0, k)][0]) == 0 for k in range(3))
    r = _run(world, c)
    _check(r, o)


# --------------------------------------------------------------------------------------------------------- 8. all gates zero
def test_all_gates_zero_is_mh_icp_align_layers(world, cases):
    c = cases["near_far_1025"]
    p = replace(_params(c), poll_every=4)  # (n_host_polls and n_enqueued_iterations are part of the struct: fixed chunks)
    pairs = world.pairs(c, gated=False)
    old = capi.icp_align_layers(pairs, world.inp.T0, p, want_pairs=True)
    assert old["n_final_pairs"] > 0
    structs = []
    for gates in (None, (capi.LayerPairGates * 3)()):
        new, raw = _align_gated_raw(pairs, world.inp.T0, p, gates)
        _bitwise(new, old)
        structs.append(raw)
    assert structs[0] == structs[1]


# --------------------------------------------------------------------------------------------------------- 9. reproducibility
def test_bitwise_equal_run_to_run_without_graphs_and_polling_every_iteration(world, cases, monkeypatch):
    c = cases["near_far_1025"]
    runs = [_run(world, c) for _ in range(3)]  # (the third one replays a captured graph)
    monkeypatch.setenv("MH_NO_GRAPH", "1")
    runs.append(_run(world, c))
    monkeypatch.delenv("MH_NO_GRAPH")
    runs.append(capi.icp_align_layers(world.pairs(c), world.inp.T0, _params(c, poll_every=1), want_pairs=True))
    assert runs[-1]["n_host_polls"] > runs[0]["n_host_polls"]
    for other in runs[1:]:
        _bitwise(other, runs[0])


# ---------------------------------------------------------------------------------------------------------- 10. hook and prior
def test_device_hook_fires_after_the_gated_pair_has_entered(world, cases, refs):
    c, o = cases["hook"], refs("hook")
    assert capi.TERM_NAMES[o["termination_reason"]] == "HookRequest" and o["n_iterations"] >= c["pairs"][0]["gate"][0]
    r = _run(world, c)
    _check(r, o)
    assert r["pair_counts"][0] > 0


def test_prior_with_a_gated_pair(world, cases, refs):
    c, o = cases["prior"], refs("prior")
    assert o["n_iterations"] > 4
    r = _run(world, c)
    _check(r, o)


# ----------------------------------------------------------------------------------------------------------- 11. host layer
# (the ICP block of tests/test_host_layer.py's near-far test: the shape of the reference's lidar3d-near-far.yaml:150-199)
_NEAR_FAR_ICP = """
class_name: mp2p_icp::ICP
params:
  maxIterations: 60
  minAbsStep_trans: 1e-4
  minAbsStep_rot: 5e-5
solvers:
  - class: mp2p_icp::Solver_GaussNewton
    params:
      maxIterations: 2
      robustKernel: 'RobustKernel::GemanMcClure'
      robustKernelParam: '0.5*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-(2.0*ADAPTIVE_THRESHOLD_SIGMA-0.5*ADAPTIVE_THRESHOLD_SIGMA)*ICP_ITERATION/30)'
matchers:
  - class: mp2p_icp::Matcher_Points_DistanceThreshold
    params:
      threshold: '2.0*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-(2.0*ADAPTIVE_THRESHOLD_SIGMA-0.5*ADAPTIVE_THRESHOLD_SIGMA)*ICP_ITERATION/30)'
      thresholdAngularDeg: 0
      pairingsPerPoint: 1
      allowMatchAlreadyMatchedGlobalPoints: true
      runFromIteration: 4
      runUpToIteration: 0
      pointLayerMatches:
        - {global: "localmap_far", local: "decimated_for_icp_far", weight: 1.0}
  - class: mp2p_icp::Matcher_Points_DistanceThreshold
    params:
      threshold: '2.00*ADAPTIVE_THRESHOLD_SIGMA'
      thresholdAngularDeg: 0
      pairingsPerPoint: 1
      allowMatchAlreadyMatchedGlobalPoints: true
      runFromIteration: 0
      runUpToIteration: %d
      pointLayerMatches:
        - {global: "localmap_near", local: "decimated_for_icp_near", weight: 1.0}
        - {global: "localmap_far", local: "decimated_for_icp_near", weight: 1.0}
quality:
  - class: mp2p_icp::QualityEvaluator_PairedRatio
    params:
      ~
"""


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


@pytest.mark.parametrize("up_to", [0, 9])
def test_host_layer_runs_gated_matchers_on_the_fused_loop(hl, oracle, inp, up_to, monkeypatch):
    monkeypatch.delenv("MOLA_HIP_FUSE_GATES", raising=False)
    hl.reload_plugin_switches()
    w, sigma = inp.w, 1.2
    far_l = np.ascontiguousarray(w.scan_xyz[np.linalg.norm(w.scan_xyz, axis=1) >= 6.0])
    g = hl.metric_map_t()
    for name, key in (("localmap_near", "near"), ("localmap_far", "far")):
        hv = hl.HashedVoxelPointCloud(inp.maps[key][1], inp.maps[key][2])
        hv.setPoints(inp.maps[key][0])
        g.set_layer(name, hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp_near", hl.PointCloud(inp.near_l))
    l.set_layer("decimated_for_icp_far", hl.PointCloud(far_l))
    icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(_NEAR_FAR_ICP % up_to))
    src = hl.ParameterSource()
    src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", sigma)
    src.updateVariable("ICP_ITERATION", 0)
    icp.attachToParameterSource(src)
    src.realize()
    assert icp.alignPath() == "generic"  # the setter off: the route it always had
    icp.fuseGatedMatchers(True)
    assert icp.alignPath() == "layers"
    fused = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert icp.lastAlignUsedFusedPath()
    icp.forceGenericPath(True)
    gen = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert not icp.lastAlignUsedFusedPath()
    np.testing.assert_allclose(fused.pose(), gen.pose(), rtol=0, atol=1e-7)
    assert fused.nIterations == gen.nIterations and fused.terminationReason == gen.terminationReason
    assert fused.potential_pairings() == gen.potential_pairings() and fused.quality == gen.quality
    assert fused.pair_local_idx() == gen.pair_local_idx() and fused.pair_global_idx() == gen.pair_global_idx()
    # ... and the reference
    base = G.base(sigma, 60)
    omaps = inp.omaps()
    pairs = [dict(map=omaps["far"], local=far_l, threshold=2.0 * base), dict(map=omaps["near"], local=inp.near_l, threshold=np.full(60, 2.0 * sigma)),
             dict(map=omaps["far"], local=inp.near_l, threshold=np.full(60, 2.0 * sigma))]
    op = oracle.ICPParams(max_iterations=60, min_abs_step_trans=1e-4, min_abs_step_rot=5e-5, kernel_param=0.5 * base,
                          gn=oracle.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))
    o = G.reference(pairs, [(4, 0), (0, up_to), (0, up_to)], w.T_guess, op)
    assert capi.TERM_NAMES[o["termination_reason"]] == fused.terminationReason.name and o["n_iterations"] == fused.nIterations
    assert o["n_iterations"] > max(4, up_to)
    np.testing.assert_allclose(fused.pose(), o["T"], rtol=0, atol=1e-7)
    assert fused.n_pairs() == o["n_final_pairs"] and fused.potential_pairings() == o["potential_pairings"]
    assert fused.quality == o["quality"]
    assert fused.pair_local_idx() == np.concatenate([q["local_idx"] for q in o["pairs"]]).tolist()
    assert fused.pair_global_idx() == np.concatenate([q["global_idx"] for q in o["pairs"]]).tolist()


# ---------------------------------------------------------------------------------------------------------------- 12. driver
# The near-far filter chain of tests/test_odometry_chains.py (copied: this file stands on its own), on the repository's default
# pipeline file with its ICP layer pairs replaced.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
_ROBOT_POSE = "[robot_x, robot_y, robot_z, robot_yaw, robot_pitch, robot_roll]"
_E = "ESTIMATED_SENSOR_MAX_RANGE"


def _map(name, cap, far="1.50"):
    return f"""  - class_name: mp2p_icp_filters::Generator
    params:
      target_layer: '{name}'
      metric_map_definition:
        class: mola::HashedVoxelPointCloud
        creationOpts:
          voxel_size: '$f{{max(0.5, 0.01*{_E})}}'
        insertOpts:
          max_points_per_voxel: {cap}
          min_distance_between_points: 0
          remove_voxels_farther_than: '$f{{max(100.0, {far}*{_E})}}'
"""


def _merge(layer, target):
    return f"""  - class_name: mp2p_icp_filters::FilterMerge
    params:
      input_pointcloud_layer: '{layer}'
      target_layer: '{target}'
      input_layer_in_local_coordinates: true
      robot_pose: {_ROBOT_POSE}
"""


def _decimate(src, dst, res):
    return f"""  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: '{src}'
      output_pointcloud_layer: '{dst}'
      voxel_filter_resolution: {res}
      decimate_method: DecimateMethod::FirstPoint
"""


# the structure of extras/lidar3d-near-far.yaml: time stamps adjusted, decimation before the de-skew of the 2nd pass
NEARFAR_TAIL = ("localmap_generator:\n" + _map("localmap_near", 20) + _map("localmap_far", 10, "1.10") + f"""observations_filter_adjust_timestamps:
  - class_name: mp2p_icp_filters::FilterAdjustTimestamps
    params:
      pointcloud_layer: 'raw'
      silently_ignore_no_timestamps: true
      time_offset: 'SENSOR_TIME_OFFSET'
      method: 'TimestampAdjustMethod::MiddleIsZero'
observations_filter_1st_pass:
  - class_name: mp2p_icp_filters::FilterByRange
    params:
      input_pointcloud_layer: 'raw'
      output_layer_between: 'filtered'
      range_min: 1.0
      range_max: 1.2*{_E}
  - class_name: mp2p_icp_filters::FilterBoundingBox
    params:
      input_pointcloud_layer: 'filtered'
      inside_pointcloud_layer: 'near'
      outside_pointcloud_layer: 'far'
      bounding_box_min: [-15.0, -15.0, -40.0]
      bounding_box_max: [15.0, 15.0, 100.0]
""" + _decimate("near", "decimated_for_icp_near_skewed", "0.75") + _decimate("near", "decimated_for_map_near_skewed", "0.25") +
                _decimate("far", "decimated_for_map_far_skewed", "0.5") + _decimate("far", "decimated_for_icp_far_skewed", "1.5") +
                """observations_filter_2nd_pass:
  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['decimated_for_map_far', 'decimated_for_icp_far', 'decimated_for_map_near', 'decimated_for_icp_near']
      error_on_missing_input_layer: false
""" + "".join(f"""  - class_name: mp2p_icp_filters::FilterDeskew
    params:
      input_pointcloud_layer: 'decimated_for_{k}_skewed'
      output_pointcloud_layer: 'decimated_for_{k}'
      silently_ignore_no_timestamps: true
""" for k in ("map_far", "icp_far", "map_near", "icp_near")) + "insert_observation_into_local_map:\n" +
                _merge("decimated_for_map_near", "localmap_near") + _merge("decimated_for_map_far", "localmap_far"))


_FAR_ENTRY = '          - {global: "localmap_far", local: "decimated_for_icp_far", weight: 1.0}\n'
_GATED_MATCHES = _FAR_ENTRY + """    - class: mp2p_icp_hip::Matcher_Points_DistanceThreshold
      params:
        threshold: '2.00*ADAPTIVE_THRESHOLD_SIGMA'
        thresholdAngularDeg: 0
        pairingsPerPoint: 1
        allowMatchAlreadyMatchedGlobalPoints: true
        pointLayerMatches:
          - {global: "localmap_near", local: "decimated_for_icp_near", weight: 1.0}
          - {global: "localmap_far", local: "decimated_for_icp_near", weight: 1.0}
"""


def _near_far_config(hl, source):
    """The reference's own lidar3d-near-far.yaml where its tree is present; `inline`: the near-far filter chain of
    tests/test_odometry_chains.py with that file's ICP block (the far pair from iteration 4, then near / near and far / near)."""
    if source == "reference":
        if not os.path.exists(REF_NEAR_FAR):
            pytest.skip("reference tree not present on this box")
        return hl.Config.FromYamlFile(REF_NEAR_FAR)
    head = open(PIPE).read().split("\nlocalmap_generator:")[0] + "\n"
    one = '          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}\n'
    assert one in head
    text = head.replace(one, _GATED_MATCHES) + NEARFAR_TAIL
    gate = "        pointLayerMatches:\n" + _FAR_ENTRY
    assert text.count(gate) >= 1
    return hl.Config.FromYamlText(text.replace(gate, "        runFromIteration: 4\n" + gate))


def _drive(hl, cfg, scans, stamps):
    lo = hl.LidarOdometry(0, True)
    lo.initialize(cfg)
    path = lo.describePipeline()["icp_path"]
    for k, (xyz, t) in enumerate(scans):
        lo.onLidar(float(stamps[k]), xyz, t)
    return path, lo.profile(), [np.asarray(r["pose"]) for r in lo.records()]


@pytest.mark.parametrize("source", ["reference", "inline"])
def test_driver_runs_gated_near_far_on_the_fused_loop(hl, monkeypatch, source):
    cfg = _near_far_config(hl, source)
    drive = synth.make_drive(14)
    scans, stamps = drive["scans"][:6], drive["stamps"][:6]
    monkeypatch.delenv("MOLA_HIP_FUSE_GATES", raising=False)
    hl.reload_plugin_switches()
    path, prof, poses = _drive(hl, cfg, scans, stamps)
    assert path == "layers"
    assert prof["icp.align_calls"] >= len(scans) - 1 and prof["icp.fused_align_calls"] == prof["icp.align_calls"]
    monkeypatch.setenv("MOLA_HIP_FUSE_GATES", "0")
    hl.reload_plugin_switches()
    try:
        path0, prof0, poses0 = _drive(hl, cfg, scans, stamps)
    finally:
        monkeypatch.delenv("MOLA_HIP_FUSE_GATES")
        hl.reload_plugin_switches()
    assert path0 == "generic" and prof0.get("icp.fused_align_calls", 0) == 0 and prof0["icp.align_calls"] == prof["icp.align_calls"]
    d = max(float(np.abs(a - b).max()) for a, b in zip(poses, poses0))
    print("%s: fused against matcher-by-matcher over %d scans: max |dT| %.3e" % (source, len(poses), d))
    assert len(poses) == len(poses0) == len(scans) and d < 1e-6
