"""allowMatchAlreadyMatchedGlobalPoints: false (U13) through the host layer: the one-matcher pipeline on the multi-layer device
loop (mh_icp_align_layers_opts) against its own matcher-by-matcher loop, which applies the claims on the host, both against the
float64 reference; and pairingsPerPoint 2, which only the matcher-by-matcher loop takes, against a first-claim filter over the
CPU oracle's k-nearest matcher."""
import numpy as np
import pytest

from mola_lidar_odometry_amd import capi, synth
from oracle import layers_oracle
from test_gpu_icp_layers import _ICP_HEAD, _MATCHER, _QUALITY, _base, _entries
from unique_global_ref import reference

pytestmark = pytest.mark.gpu

_SCHEDULE = "2.0*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-(2.0*ADAPTIVE_THRESHOLD_SIGMA-0.5*ADAPTIVE_THRESHOLD_SIGMA)*ICP_ITERATION/30)"
ONE_UNIQUE = (_ICP_HEAD + _MATCHER % (_SCHEDULE, _entries([("localmap", "decimated_for_icp")])) + _QUALITY).replace(
    "allowMatchAlreadyMatchedGlobalPoints: true", "allowMatchAlreadyMatchedGlobalPoints: false")
TWO_PER_POINT = (_ICP_HEAD.replace("maxIterations: 40", "maxIterations: 1") +
                 _MATCHER % ("2.0", _entries([("localmap", "decimated_for_icp")])) + _QUALITY).replace(
    "allowMatchAlreadyMatchedGlobalPoints: true", "allowMatchAlreadyMatchedGlobalPoints: false").replace(
    "pairingsPerPoint: 1", "pairingsPerPoint: 2")


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


def _layers(hl, w):
    g = hl.metric_map_t()
    hv = hl.HashedVoxelPointCloud(w.voxel_size, w.cap)
    hv.setPoints(w.map_xyz)
    g.set_layer("localmap", hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp", hl.PointCloud(w.scan_xyz))
    return l, g


def _icp(hl, w, text, generic):
    icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(text))
    src = hl.ParameterSource()
    src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", w.sigma)
    src.updateVariable("ICP_ITERATION", 0)
    icp.attachToParameterSource(src)
    src.realize()
    icp.forceGenericPath(generic)
    return icp, params, src  # the ICP refers to the source without owning it: the caller keeps it alive across align()


def test_one_unique_matcher_fused_equals_its_generic_loop_and_the_reference(hl, oracle, small_workload):
    w = small_workload
    assert "allowMatchAlreadyMatchedGlobalPoints: false" in ONE_UNIQUE
    l, g = _layers(hl, w)
    out = {}
    for generic in (False, True):
        icp, params, src = _icp(hl, w, ONE_UNIQUE, generic)
        assert icp.alignPath() == ("generic" if generic else "layers")
        out[generic] = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
        assert icp.lastAlignUsedFusedPath() == (not generic)
    a, b = out[False], out[True]
    assert a.nIterations == b.nIterations and a.terminationReason.name == b.terminationReason.name
    assert a.n_pairs() == b.n_pairs()
    np.testing.assert_array_equal(np.asarray(a.pair_global_idx()), np.asarray(b.pair_global_idx()))
    np.testing.assert_allclose(a.pose(), b.pose(), rtol=0, atol=1e-7)
    b40 = _base(w.sigma, 40)
    o = reference([dict(map=oracle.Map(w.voxel_size, w.cap).insert(w.map_xyz), local=w.scan_xyz, threshold=2.0 * b40)], [1],
                  synth.pose_from_ypr(w.guess_ypr),
                  oracle.ICPParams(max_iterations=40, kernel_param=0.5 * b40, gn=oracle.GNParams(max_inner_iterations=2)))
    assert o["dropped"] >= 0.2 * o["candidates"] and layers_oracle.nearest_decision(o["margins"])[1] > 1e-6
    for res in (a, b):
        assert res.nIterations == o["n_iterations"] and res.terminationReason.name == capi.TERM_NAMES[o["termination_reason"]]
        assert res.n_pairs() == o["n_final_pairs"] > 0
        assert res.quality == pytest.approx(o["quality"], abs=1e-12)
        np.testing.assert_array_equal(np.asarray(res.pair_local_idx()), o["pairs"][0]["local_idx"])
        np.testing.assert_array_equal(np.asarray(res.pair_global_idx()), o["pairs"][0]["global_idx"])
        np.testing.assert_allclose(res.pose(), o["T"], rtol=0, atol=1e-7)


def test_two_pairings_per_point_claim_one_by_one_in_the_generic_loop(hl, oracle, small_workload):
    """pairingsPerPoint 2: each of a point's two accepted candidates is tested and claims on its own, in the order the matcher
    lists them.  One iteration (maxIterations 1): the final pairings are those of the initial guess.  Threshold 2.0: all 4000
    candidates of the 2000-point scan are accepted and name 1676 distinct map points."""
    w = small_workload
    l, g = _layers(hl, w)
    icp, params, src = _icp(hl, w, TWO_PER_POINT, False)
    assert icp.alignPath() == "generic"
    res = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    m = oracle.match_points_k(oracle.Map(w.voxel_size, w.cap).insert(w.map_xyz), w.scan_xyz, synth.pose_from_ypr(w.guess_ypr), 2.0, 2)
    _, first = np.unique(m["global_idx"], return_index=True)  # the first candidate naming each map point, in matching order
    keep = np.sort(first)
    print("candidates %d, distinct map points %d" % (len(m["global_idx"]), len(keep)))
    assert (len(m["global_idx"]), len(keep)) == (4000, 1676)
    np.testing.assert_array_equal(np.asarray(res.pair_local_idx()), m["local_idx"][keep])
    np.testing.assert_array_equal(np.asarray(res.pair_global_idx()), m["global_idx"][keep])
