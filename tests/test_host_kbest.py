"""pairingsPerPoint > 1 through the host layer: routing (ICP::fuseMultiPairings, MOLA_HIP_FUSE_KBEST) on the CPU; on the device the
fused route (mh_icp_align_layers_kbest) against the matcher-by-matcher one and against the oracle's loop, and the stand-alone driver
on the default pipeline file with pairingsPerPoint: 2."""
import os

import numpy as np
import pytest

import kbest_ref as kr
from mola_lidar_odometry_amd import capi, synth
from oracle import layers_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")

_HEAD = """
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
      robustKernelParam: 0.3
matchers:
"""

_TAIL = """quality:
  - class: mp2p_icp::QualityEvaluator_PairedRatio
    params:
      ~
"""


def _points(entries, ppp=2, run_from=0, allow=True, thr="0.9", ang="0.5"):
    lines = ["  - class: mp2p_icp::Matcher_Points_DistanceThreshold", "    params:", f"      threshold: {thr}",
             f"      thresholdAngularDeg: {ang}", f"      pairingsPerPoint: {ppp}",
             f"      allowMatchAlreadyMatchedGlobalPoints: {'true' if allow else 'false'}", f"      runFromIteration: {run_from}",
             "      pointLayerMatches:"]
    lines += [f'        - {{global: "{g}", local: "{l}", weight: 1.0}}' for g, l in entries]
    return "\n".join(lines) + "\n"


_ONE = [("localmap", "decimated_for_icp")]
TWO = _HEAD + _points(_ONE) + _TAIL  # the text of tests/test_host_layer.py's pairingsPerPoint: 2 pipeline
TWO_GATED = _HEAD + _points(_ONE, run_from=2) + _points([("localmap", "other")], ppp=1) + _TAIL
TWO_UNIQUE = _HEAD + _points(_ONE, allow=False) + _TAIL
NINE = _HEAD + _points(_ONE, ppp=9) + _TAIL


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


@pytest.fixture
def kbest_env(hl):
    """MOLA_HIP_FUSE_KBEST / MOLA_HIP_FUSE_GATES for the duration of a test (the library caches its switches)."""
    names = ("MOLA_HIP_FUSE_KBEST", "MOLA_HIP_FUSE_GATES")
    old = {n: os.environ.get(n) for n in names}

    def set_(kbest, gates=None):
        for n, v in zip(names, (kbest, gates)):
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        hl.reload_plugin_switches()
    yield set_
    set_(*[old[n] for n in names])


def _icp(hl, text, kbest=None, gates=None):
    icp, _ = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(text))
    if kbest is not None:
        icp.fuseMultiPairings(kbest)
    if gates is not None:
        icp.fuseGatedMatchers(gates)
    return icp


# ------------------------------------------------------------------------------------------------------------- routing (CPU)
def test_setter_and_environment_override(hl, kbest_env):
    kbest_env(None)
    assert hl.plugin_switch_fuse_kbest() == -1
    assert _icp(hl, TWO).alignPath() == "generic"  # the default: off
    assert _icp(hl, TWO, True).alignPath() == "layers"  # a single pair qualifies
    assert _icp(hl, TWO, False).alignPath() == "generic"
    kbest_env("1")  # the environment wins, both ways
    assert hl.plugin_switch_fuse_kbest() == 1
    assert _icp(hl, TWO).alignPath() == "layers" and _icp(hl, TWO, False).alignPath() == "layers"
    kbest_env("0")
    assert hl.plugin_switch_fuse_kbest() == 0
    assert _icp(hl, TWO, True).alignPath() == "generic"
    kbest_env(None)
    icp = _icp(hl, TWO, True)
    icp.forceGenericPath(True)
    assert icp.alignPath() == "generic"


def test_with_a_gate_and_with_unique_map_points(hl, kbest_env):
    kbest_env(None)
    assert _icp(hl, TWO_GATED).alignPath() == "generic"
    assert _icp(hl, TWO_GATED, True).alignPath() == "generic"  # the gate has a switch of its own
    assert _icp(hl, TWO_GATED, False, True).alignPath() == "generic"
    assert _icp(hl, TWO_GATED, True, True).alignPath() == "layers"
    kbest_env("1", "1")
    assert _icp(hl, TWO_GATED).alignPath() == "layers"
    kbest_env("1", "0")
    assert _icp(hl, TWO_GATED, True, True).alignPath() == "generic"
    kbest_env(None)
    assert _icp(hl, TWO_UNIQUE).alignPath() == "generic"
    assert _icp(hl, TWO_UNIQUE, True).alignPath() == "layers"
    kbest_env("0")
    assert _icp(hl, TWO_UNIQUE, True).alignPath() == "generic"


def test_nine_pairings_per_point_throw_as_before(hl, kbest_env):
    for env in (None, "1"):
        kbest_env(env)
        with pytest.raises(RuntimeError, match="pairingsPerPoint"):
            _icp(hl, NINE, True).alignPath()


# ----------------------------------------------------------------------------------------------------------- fused vs generic
@pytest.mark.gpu
def test_fused_and_generic_routes_match_the_oracle_loop(hl, oracle, small_workload, kbest_env):
    kbest_env(None)
    w = small_workload
    g = hl.metric_map_t()
    hv = hl.HashedVoxelPointCloud(1.0, 20)
    hv.setPoints(w.map_xyz)
    g.set_layer("localmap", hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp", hl.PointCloud(w.scan_xyz))
    icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(TWO))
    assert icp.alignPath() == "generic"
    gen = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert not icp.lastAlignUsedFusedPath()
    icp.fuseMultiPairings(True)
    assert icp.alignPath() == "layers"
    fused = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
    assert icp.lastAlignUsedFusedPath()
    # the reference: the float64 loop over the k-nearest matcher
    om = oracle.Map(1.0, 20).insert(w.map_xyz)
    op = oracle.ICPParams(max_iterations=40, min_abs_step_trans=1e-4, min_abs_step_rot=5e-5, kernel_param=np.full(40, 0.3),
                          gn=oracle.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))
    o = kr.reference([dict(map=om, local=w.scan_xyz, threshold=np.full(40, 0.9), threshold_angular_deg=0.5)], [2], w.T_guess, op)
    assert not kr.set_apart(o) and o["n_final_pairs"] > 2000
    for name, res in (("fused", fused), ("generic", gen)):
        d = float(np.abs(np.asarray(res.pose()) - o["T"]).max())
        print("%s: %d iterations, %d pairings of %d, max |dT| against the reference %.2e" % (
            name, res.nIterations, res.n_pairs(), res.potential_pairings(), d))
        assert capi.TERM_NAMES[o["termination_reason"]] == res.terminationReason.name and o["n_iterations"] == res.nIterations
        assert res.n_pairs() == o["n_final_pairs"] and res.potential_pairings() == o["potential_pairings"] == 4000
        assert res.quality == o["quality"]
        assert d < 1e-7
        assert res.pair_local_idx() == o["pairs"][0]["local_idx"].tolist()
        assert res.pair_global_idx() == o["pairs"][0]["global_idx"].tolist()
    np.testing.assert_allclose(fused.pose(), gen.pose(), rtol=0, atol=1e-7)
    assert fused.n_pairs() == gen.n_pairs() and fused.potential_pairings() == gen.potential_pairings()


# ---------------------------------------------------------------------------------------------------------------------- driver
_DECISIONS = ("dropped", "first_scan", "icp_run", "icp_good", "had_motion_model", "map_updated", "restarted", "icp_iterations",
              "twist_corrections", "align_calls", "termination", "n_raw", "n_for_map", "n_for_icp", "n_map_points", "n_map_voxels")


def _drive(hl, cfg, scans, stamps):
    lo = hl.LidarOdometry(0, True)
    lo.initialize(cfg)
    path = lo.describePipeline()["icp_path"]
    for k, (xyz, t) in enumerate(scans):
        lo.onLidar(float(stamps[k]), xyz, t)
    return path, lo.profile(), lo.records()


@pytest.mark.gpu
def test_driver_runs_two_pairings_per_point_on_the_fused_loop(hl, kbest_env, tmp_path):
    text = open(PIPE).read()
    assert text.count("pairingsPerPoint: 1") >= 1
    copy = tmp_path / "lidar3d-default-k2.yaml"
    copy.write_text(text.replace("pairingsPerPoint: 1", "pairingsPerPoint: 2"))
    cfg = hl.Config.FromYamlFile(str(copy))
    drive = synth.make_drive(14)
    scans, stamps = drive["scans"][:6], drive["stamps"][:6]
    kbest_env(None)
    path, prof, recs = _drive(hl, cfg, scans, stamps)
    assert path == "layers" and prof["icp.align_calls"] >= len(scans) - 1
    assert prof["icp.host_polls"] >= prof["icp.align_calls"]  # the device loop was polled: the fused route ran
    kbest_env("0")
    path0, prof0, recs0 = _drive(hl, cfg, scans, stamps)
    assert path0 == "generic" and prof0["icp.align_calls"] == prof["icp.align_calls"]
    assert len(recs) == len(recs0) == len(scans)
    for a, b in zip(recs, recs0):
        for key in _DECISIONS:
            assert a[key] == b[key], key
    d = max(float(np.abs(np.asarray(a["pose"]) - np.asarray(b["pose"])).max()) for a, b in zip(recs, recs0))
    print("fused against matcher-by-matcher over %d scans: max |dT| %.3e" % (len(recs), d))
    assert d < 1e-6
