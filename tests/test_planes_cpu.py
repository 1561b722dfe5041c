"""Matcher_Point2Plane pairs on the multi-layer loop, CPU side: the fixed cases of tests/planes_ref.py on the reference alone -- none is
set apart by tools/fuzz_layers.py's rule (so tests/test_gpu_icp_layers_planes.py may hold the device to them), each has the property
it is there for -- the binding's signature, and the host layer's routing (ICP::fusePlaneMatchers, MOLA_HIP_FUSE_PLANES)."""
import ctypes as C
import os

import numpy as np
import pytest

import planes_ref as pr
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c


@pytest.fixture(scope="module")
def inp(small_workload, oracle):
    return pr.Inputs(small_workload)


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def refs(inp, omaps):
    return {name: (c, pr.case_reference(c, omaps)) for name, c in pr.cases(inp).items()}


def test_no_fixed_case_is_set_apart(refs):
    for name, (c, o) in refs.items():
        near = layers_oracle.nearest_decision(o["margins"])
        print("%-14s iterations %2d, final pairs %5d (plane %4d) of %5d, max cond %.2e, nearest decision %s" % (
            name, o["n_iterations"], o["n_final_pairs"], o["n_final_pairs_pt2pl"], o["potential_pairings"], o["max_cond"], near))
        assert not pr.set_apart(o), name
        assert o["max_cond"] < 1e10 and near[1] > 1e-9, (name, near)


def test_every_plane_pair_has_final_pairings(refs, inp, omaps):
    for name, (c, o) in refs.items():
        for e, cnt in zip(c["pairs"], o["pair_counts"]):
            if e["plane"]:
                assert cnt > 0, name
        assert o["n_final_pairs_pt2pl"] == sum(cnt for e, cnt in zip(c["pairs"], o["pair_counts"]) if e["plane"])
    # the one point of s[:1] has no plane pairing from the workload's guess (it has one near the true pose, where the small
    # slices start)
    c, o = refs["ref_n1"]
    assert o["pair_counts"][0] == 1
    e = c["pairs"][0]
    for T, want in ((inp.T0, 0), (inp.w.T_gt, 1), (inp.T_near, 1)):
        assert len(pr.match_plane(omaps["whole"], e["local"], T, 0.4, e["plane"])["local_idx"]) == want


def test_each_case_has_its_property(refs, omaps):
    c, o = refs["sparse"]  # most points fail minimum_plane_points: fewer than 4 records of the block inside the wide radius
    e = c["pairs"][0]
    assert 0 < o["pair_counts"][0] < 100 and len(e["local"]) == 2000
    near = oracle_c.match_points_k(omaps["sparse"], e["local"], o["poses"][-1], e["plane"]["search_radius"],
                                   e["plane"]["minimum_plane_points"])
    enough = np.bincount(near["local_idx"], minlength=2000) >= e["plane"]["minimum_plane_points"]
    print("sparse: %d of 2000 points have %d records inside the radius" % (int(enough.sum()), e["plane"]["minimum_plane_points"]))
    assert o["pair_counts"][0] <= enough.sum() < 1000
    c, o = refs["off_pose"]  # the plane index set changes between iterations
    sets = [d[0] for d in o["plane_sets"]]
    assert len(sets) == 12 and any(not np.array_equal(a, b) for a, b in zip(sets, sets[1:]))
    c, o = refs["gated"]  # nothing before the gate opens, and nothing of it in the counts
    assert [len(d[0]) for d in o["plane_sets"][:3]][:2] == [0, 0] and len(o["plane_sets"][2][0]) > 0
    c, o = refs["rgbd"]
    assert o["potential_pairings"] == 1000 * 2 + 1000 and o["pair_counts"][1] == o["n_final_pairs_pt2pl"] > 300
    c, o = refs["knn16"]
    assert c["pairs"][0]["plane"]["knn"] == capi.MAX_PLANE_KNN and o["n_final_pairs"] > 1000
    c, o = refs["dup"]  # equal distances, ordered by scan position: the covariance of a doubled point set still gives planes
    assert o["pair_counts"][0] > 100


def test_binding_signature():
    """the declared argtypes of mh_icp_align_layers_planes: kbest's with the planes array and the plane outputs"""
    f = capi.lib().mh_icp_align_layers_planes
    k = capi.lib().mh_icp_align_layers_kbest
    assert f.restype is C.c_int32
    assert list(f.argtypes[:5]) == list(k.argtypes[:5]) and f.argtypes[5] is C.POINTER(capi.LayerPairPlane)
    assert list(f.argtypes[6:12]) == list(k.argtypes[5:11]) and f.argtypes[12] is C.POINTER(capi.PairsPlOut)
    assert list(f.argtypes[13:]) == list(k.argtypes[11:])
    assert C.sizeof(capi.LayerPairPlane) == 24


# ------------------------------------------------------------------------------------------------------------------- routing
RGBD_BLOCK = """
class_name: mp2p_icp::ICP
params:
  maxIterations: 40
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
        - {global: "edges_map", local: "edges", weight: 1.0}
  - class: mp2p_icp::Matcher_Point2Plane
    params:
      distanceThreshold: 0.40
      planeEigenThreshold: 1e-2
      searchRadius: 0.80
      knn: 10
      minimumPlanePoints: 6
      pointLayerMatches:
        - {global: "planes_map", local: "planes", weight: 1.0}
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


@pytest.fixture
def planes_env(hl):
    """MOLA_HIP_FUSE_PLANES / MOLA_HIP_FUSE_KBEST for the duration of a test (the library caches its switches)."""
    names = ("MOLA_HIP_FUSE_PLANES", "MOLA_HIP_FUSE_KBEST")
    old = {n: os.environ.get(n) for n in names}

    def set_(planes, kbest=None):
        for n, v in zip(names, (planes, kbest)):
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        hl.reload_plugin_switches()
    yield set_
    set_(*[old[n] for n in names])


def rgbd_icp(hl, planes=None):
    icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(RGBD_BLOCK))
    icp.fuseMultiPairings(True)  # (the block's point matcher has pairingsPerPoint 2: a switch of its own)
    if planes is not None:
        icp.fusePlaneMatchers(planes)
    return icp, params


def test_routing_of_the_rgbd_block(hl, planes_env):
    planes_env(None)
    assert hl.plugin_switch_fuse_planes() == -1
    assert rgbd_icp(hl)[0].alignPath() == "generic"  # the default: off
    assert rgbd_icp(hl, True)[0].alignPath() == "layers"
    assert rgbd_icp(hl, False)[0].alignPath() == "generic"
    planes_env("0")
    assert hl.plugin_switch_fuse_planes() == 0
    assert rgbd_icp(hl)[0].alignPath() == "generic" and rgbd_icp(hl, True)[0].alignPath() == "generic"
    planes_env("1")  # the environment wins, both ways
    assert hl.plugin_switch_fuse_planes() == 1
    assert rgbd_icp(hl)[0].alignPath() == "layers" and rgbd_icp(hl, False)[0].alignPath() == "layers"
    icp = rgbd_icp(hl)[0]
    icp.forceGenericPath(True)
    assert icp.alignPath() == "generic"
    icp = rgbd_icp(hl)[0]
    icp.setIterationHook(lambda k, T: False)
    assert icp.alignPath() == "generic"
    planes_env("1", "0")  # the point matcher's pairingsPerPoint 2 keeps its own switch
    assert rgbd_icp(hl)[0].alignPath() == "generic"
