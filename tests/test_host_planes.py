"""Matcher_Point2Plane on point layers through the host layer, on the device: the rgbd-shaped block (a Matcher_Points_DistanceThreshold
with pairingsPerPoint 2 on the edge layers, a Matcher_Point2Plane with KNN + PCA on the plane layers, one Solver_GaussNewton) through
ICP::align on the fused route (mh_icp_align_layers_planes) and on the matcher-by-matcher one.  The routing itself is checked on the
CPU (tests/test_planes_cpu.py)."""
import numpy as np
import pytest

from test_planes_cpu import RGBD_BLOCK, hl, planes_env, rgbd_icp  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_fused_and_generic_routes_agree_on_the_rgbd_block(hl, small_workload, planes_env):
    planes_env(None)
    w = small_workload
    g = hl.metric_map_t()
    for name, pts in (("edges_map", w.map_xyz), ("planes_map", np.ascontiguousarray(w.map_xyz[::2]))):
        hv = hl.HashedVoxelPointCloud(1.0, 20)
        hv.setPoints(pts)
        g.set_layer(name, hv)
    l = hl.metric_map_t()
    l.set_layer("edges", hl.PointCloud(np.ascontiguousarray(w.scan_xyz[0::2])))
    l.set_layer("planes", hl.PointCloud(np.ascontiguousarray(w.scan_xyz[1::2])))
    icp, params = rgbd_icp(hl)
    assert icp.alignPath() == "generic"
    gen = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert not icp.lastAlignUsedFusedPath()
    icp.fusePlaneMatchers(True)
    assert icp.alignPath() == "layers"
    fused = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert icp.lastAlignUsedFusedPath()
    for name, res in (("fused", fused), ("generic", gen)):
        print("%s: %d iterations, %s, %d pairings (%d plane) of %d" % (
            name, res.nIterations, res.terminationReason.name, res.n_pairs(), res.n_pairs_pt2pl(), res.potential_pairings()))
    assert fused.nIterations == gen.nIterations > 3 and fused.terminationReason == gen.terminationReason
    assert fused.n_pairs() == gen.n_pairs() and fused.n_pairs_pt2pl() == gen.n_pairs_pt2pl() > 100
    assert fused.potential_pairings() == gen.potential_pairings() == 1000 * 2 + 1000
    assert fused.quality == gen.quality
    assert fused.pair_local_idx() == gen.pair_local_idx() and fused.pair_global_idx() == gen.pair_global_idx()
    pf, pg = np.asarray(fused.pairs_pt2pl(), np.float32), np.asarray(gen.pairs_pt2pl(), np.float32)
    np.testing.assert_array_equal(pf[:, :3], pg[:, :3])  # the same local points, in the same order: the index set
    np.testing.assert_allclose(pf[:, 3:], pg[:, 3:], rtol=0, atol=1e-6)  # centroids and normals
    np.testing.assert_allclose(fused.pose(), gen.pose(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(np.asarray(fused.cov()), np.asarray(gen.cov()), rtol=2e-5, atol=1e-6 * np.abs(np.asarray(gen.cov())).max())


def test_an_ndt_global_layer_keeps_the_generic_route(hl, small_workload, planes_env):
    """Matcher_Point2Plane means the per-voxel planes there (mh_nn_search_pt2pl): not what the loop runs."""
    planes_env(None)
    w = small_workload
    g = hl.metric_map_t()
    hv = hl.HashedVoxelPointCloud(1.0, 20)
    hv.setPoints(w.map_xyz)
    g.set_layer("edges_map", hv)
    ndt = hl.NDT(1.0, 0, 0.2, 0.05)
    ndt.setPoints(w.map_xyz)
    g.set_layer("planes_map", ndt)
    l = hl.metric_map_t()
    l.set_layer("edges", hl.PointCloud(np.ascontiguousarray(w.scan_xyz[0::2])))
    l.set_layer("planes", hl.PointCloud(np.ascontiguousarray(w.scan_xyz[1::2])))
    icp, params = rgbd_icp(hl, True)
    assert icp.alignPath() == "layers"
    r = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert not icp.lastAlignUsedFusedPath() and r.n_pairs() > 0
