"""CPU checks of the iteration gates on the fused multi-layer loop (mh_icp_align_layers_gated).

The reference alone, over exactly the inputs tests/test_gpu_icp_layers_gates.py runs on the device (tests/gates_ref.py): no case
may be "set apart" by the rule of tools/fuzz_layers.py (a stall / hook / min_delta / max_cost decision within 1e-9, relative, of
its threshold, or normal equations conditioned above 1e10) -- the cap is zero cases -- and the gates matter in every one of them:
the pairing counts of the gated iterations differ from the ungated alignment's and the final pose lies more than 1e-4 from it (the
margin tests/test_gpu_solver_params.py uses for "a parameter matters").  Then the host layer's routing (setter, environment
override, shapes that stay where they were), and the boundary of the new entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gates_ref as G
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")

# the ICP block shapes of tests/test_icp_layers_routing.py (copied: this file stands on its own)
_HEAD = """
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
      robustKernelParam: '0.5*ADAPTIVE_THRESHOLD_SIGMA'
matchers:
"""

_TAIL = """quality:
  - class: mp2p_icp::QualityEvaluator_PairedRatio
    params:
      ~
"""


def _points(thr, entries, run_from=0, up_to=0, ppp=1):
    lines = ["  - class: mp2p_icp::Matcher_Points_DistanceThreshold", "    params:", f"      threshold: '{thr}'",
             "      thresholdAngularDeg: 0", f"      pairingsPerPoint: {ppp}", "      allowMatchAlreadyMatchedGlobalPoints: true",
             f"      runFromIteration: {run_from}", f"      runUpToIteration: {up_to}", "      pointLayerMatches:"]
    lines += [f'        - {{global: "{g}", local: "{l}", weight: {w}}}' for g, l, w in entries]
    return "\n".join(lines) + "\n"


def _plane(entries, run_from=0):
    lines = ["  - class: mp2p_icp::Matcher_Point2Plane", "    params:", "      distanceThreshold: '1.0*ADAPTIVE_THRESHOLD_SIGMA'",
             f"      runFromIteration: {run_from}", "      runUpToIteration: 0", "      pointLayerMatches:"]
    lines += [f'        - {{global: "{g}", local: "{l}", weight: 1.0}}' for g, l in entries]
    return "\n".join(lines) + "\n"


_S2 = "2.0*ADAPTIVE_THRESHOLD_SIGMA"
DUAL_MAP = _HEAD + _points("3.0*ADAPTIVE_THRESHOLD_SIGMA", [("localmap", "decimated_for_icp", 1.0)]) + \
    _points(_S2, [("localmap_far", "decimated_for_icp_near", 1.0)]) + _TAIL
EDGES = _HEAD + _points(_S2, [("map_large_curv", "scan_large_curv", 1.0), ("map_small_curv", "scan_small_curv", 1.0)]) + _TAIL
NEAR_FAR = _HEAD + _points(_S2, [("localmap_far", "decimated_for_icp_far", 1.0)], run_from=4) + \
    _points(_S2, [("localmap_near", "decimated_for_icp_near", 1.0), ("localmap_far", "decimated_for_icp_near", 1.0)]) + _TAIL
TWO_PER_POINT = _HEAD + _points(_S2, [("a", "x", 1.0), ("b", "y", 1.0)], ppp=2) + _TAIL
DEFAULT = _HEAD + _points(_S2, [("localmap", "decimated_for_icp", 1.0)]) + _TAIL
NDT = _HEAD + _plane([("localmap", "decimated_for_icp")]) + _points(_S2, [("localmap", "decimated_for_icp", 1.0)]) + _TAIL


# ------------------------------------------------------------------------------------------------------- the reference alone
@pytest.fixture(scope="module")
def inp(small_workload):
    return G.Inputs(small_workload)


@pytest.fixture(scope="module")
def omaps(oracle, inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def cases(inp):
    return G.cases(inp)


def test_the_case_list_is_what_the_gpu_file_runs(cases):
    assert set(G.CASES_1_TO_7) | {"hook", "prior"} == set(cases)


@pytest.mark.parametrize("name", G.CASES_1_TO_7 + ["hook", "prior"])
def test_no_case_is_set_apart(inp, omaps, cases, name):
    o = G.case_reference(cases[name], omaps, inp.T0)
    nd = layers_oracle.nearest_decision(o["margins"])
    print("%s: nearest decision %s, max condition number %.2e" % (name, nd, o["max_cond"]))
    assert nd is None or nd[1] > 1e-9
    assert o["max_cond"] <= 1e10


@pytest.mark.parametrize("name", G.CASES_1_TO_7)
def test_the_gates_matter(inp, omaps, cases, name):
    c = cases[name]
    o = G.case_reference(c, omaps, inp.T0)
    full = G.case_reference(dict(c, without=None), omaps, inp.T0, gated=False)  # the same pairs, no gates
    shift = float(np.abs(o["T"] - full["T"]).max())
    tr, tf = [t["n_pairs"] for t in o["trace"]], [t["n_pairs"] for t in full["trace"]]
    print("%s: pose shift against the ungated alignment %.3e; n_pairs %s against %s" % (name, shift, tr[:8], tf[:8]))
    assert shift > 1e-4
    gates = [e["gate"] for e in c["pairs"]]
    gated_its = [k for k in range(max(len(tf), len(tr))) if not all(G.active(g, k) for g in gates)]
    assert gated_its
    for k in gated_its[:min(len(gated_its), 8)]:
        if k < len(tf):
            assert k >= len(tr) or tr[k] != tf[k], k  # (k >= len(tr): the gated loop has ended by then)
    if c["without"] is not None:
        # a pair that never runs: the alignment that lacks it, number for number (here the reference is exact against itself)
        lacking = G.case_reference(c, omaps, inp.T0, gated=False)
        np.testing.assert_array_equal(o["T"], lacking["T"])
        assert tr == [t["n_pairs"] for t in lacking["trace"]] and o["n_iterations"] == lacking["n_iterations"]
        assert o["potential_pairings"] == lacking["potential_pairings"] and o["quality"] == lacking["quality"]
        assert [k for i, k in enumerate(o["pair_counts"]) if i in c["without"]] == lacking["pair_counts"]


def test_potential_pairings_follow_the_last_match(inp, omaps, cases):
    n_near, n_far = len(inp.near_l), 1360
    o = G.case_reference(cases["up_to"], omaps, inp.T0)
    assert o["potential_pairings"] == n_far and o["quality"] == o["n_final_pairs"] / n_far
    o = G.case_reference(cases["nobody_at_3"], omaps, inp.T0)
    assert (o["n_iterations"], o["potential_pairings"], o["quality"]) == (3, 0, 0.0)
    o = G.case_reference(cases["near_far_65"], omaps, inp.T0)
    assert o["potential_pairings"] == 65 + 2 * n_near


# ------------------------------------------------------------------------------------------------------------------- routing
@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


@pytest.fixture
def fuse_gates_env(hl):
    """MOLA_HIP_FUSE_GATES for the duration of a test (the library caches its switches)."""
    old = os.environ.get("MOLA_HIP_FUSE_GATES")

    def set_(v):
        if v is None:
            os.environ.pop("MOLA_HIP_FUSE_GATES", None)
        else:
            os.environ["MOLA_HIP_FUSE_GATES"] = v
        hl.reload_plugin_switches()
    yield set_
    set_(old)


def _icp(hl, text, setter=None):
    icp, _ = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(text))
    if setter is not None:
        icp.fuseGatedMatchers(setter)
    return icp


def test_setter_and_environment_override(hl, fuse_gates_env):
    fuse_gates_env(None)
    assert hl.plugin_switch_fuse_gates() == -1
    assert _icp(hl, NEAR_FAR).alignPath() == "generic"          # the default: off
    assert _icp(hl, NEAR_FAR, True).alignPath() == "layers"
    assert _icp(hl, NEAR_FAR, False).alignPath() == "generic"
    fuse_gates_env("1")                                          # the environment wins, both ways
    assert hl.plugin_switch_fuse_gates() == 1
    assert _icp(hl, NEAR_FAR).alignPath() == "layers" and _icp(hl, NEAR_FAR, False).alignPath() == "layers"
    fuse_gates_env("0")
    assert _icp(hl, NEAR_FAR, True).alignPath() == "generic"
    fuse_gates_env(None)
    icp = _icp(hl, NEAR_FAR, True)
    icp.forceGenericPath(True)
    assert icp.alignPath() == "generic"


@pytest.mark.parametrize("text, want", [(DUAL_MAP, "layers"), (EDGES, "layers"), (NEAR_FAR, "generic"), (TWO_PER_POINT, "generic"),
                                        (DEFAULT, "single"), (NDT, "single")],
                         ids=["dual-map", "edges", "near-far", "pairingsPerPoint-2", "default", "ndt"])
def test_every_shape_keeps_its_path_with_the_setter_off(hl, fuse_gates_env, text, want):
    fuse_gates_env(None)
    assert _icp(hl, text).alignPath() == want
    assert _icp(hl, text, False).alignPath() == want
    if text is not NEAR_FAR:  # ... and the ungated ones with it on
        assert _icp(hl, text, True).alignPath() == want


def test_gated_shapes_the_fused_loop_takes_and_leaves(hl, fuse_gates_env):
    fuse_gates_env(None)
    one_gated = _HEAD + _points("2.0", [("a", "x", 1.0)], run_from=4) + _TAIL           # a single gated pair: the layers loop
    up_to = _HEAD + _points("2.0", [("a", "x", 1.0), ("b", "y", 1.0)], up_to=9) + _TAIL
    two_per_point = _HEAD + _points("2.0", [("a", "x", 1.0), ("b", "y", 1.0)], run_from=4, ppp=2) + _TAIL
    nine = _HEAD + _points("2.0", [(f"g{i}", f"l{i}", 1.0) for i in range(9)], run_from=2) + _TAIL
    assert _icp(hl, one_gated, True).alignPath() == "layers" and _icp(hl, one_gated).alignPath() == "generic"
    assert _icp(hl, up_to, True).alignPath() == "layers" and _icp(hl, up_to).alignPath() == "generic"
    assert _icp(hl, two_per_point, True).alignPath() == "generic"
    assert _icp(hl, nine, True).alignPath() == "generic"
    plane_gated = _HEAD + _plane([("localmap", "decimated_for_icp")], run_from=2) + _points("2.0", [("localmap", "decimated_for_icp", 1.0)]) + _TAIL
    assert _icp(hl, plane_gated, True).alignPath() == "generic"


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_gates_struct_layout_matches_c(tmp_path):
    prog = tmp_path / "lg.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %d\n", sizeof(mh_layer_pair_gates), offsetof(mh_layer_pair_gates, run_from_iteration),
    offsetof(mh_layer_pair_gates, run_up_to_iteration), sizeof(mh_layer_pair_opts), offsetof(mh_layer_pair_opts, unique_global),
    MH_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "lg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    g, o = capi.LayerPairGates, capi.LayerPairOpts
    assert vals[:3] == [C.sizeof(g), g.run_from_iteration.offset, g.run_up_to_iteration.offset] == [8, 0, 4]
    assert vals[3:5] == [C.sizeof(o), o.unique_global.offset]          # mh_layer_pair_opts keeps its layout ...
    assert vals[5] == int(capi.lib().mh_abi_version())                 # ... so the ABI version has not moved


def test_entry_point_is_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"MH_API\s+mh_status\s+mh_icp_align_layers_gated\s*\(", text)
    assert "mh_icp_align_layers_gated" in capi._SIGNATURES and hasattr(capi.lib(), "mh_icp_align_layers_gated")
    restype, argtypes = capi._SIGNATURES["mh_icp_align_layers_gated"]
    assert restype is C.c_int32 and len(argtypes) == 12 and argtypes[3] is C.POINTER(capi.LayerPairGates)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib()._name], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mh_icp_align_layers_gated$", out, re.M)
