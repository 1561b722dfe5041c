"""CPU checks of allowMatchAlreadyMatchedGlobalPoints: false (U13): the boundary of mh_icp_align_layers_opts -- declaration,
export, binding, an unchanged ABI version -- and the host layer's routing of pipelines that write the key."""
import re
import subprocess

import pytest

from mola_lidar_odometry_amd import capi
from test_icp_layers_routing import _HEAD, _TAIL, _points


def test_entry_point_is_declared_exported_and_bound():
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "molahip.h")
    text = open(header).read()
    assert re.search(r"MH_API\s+mh_status\s+mh_icp_align_layers_opts\s*\(", text)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+unique_global;[^}]*\}\s*mh_layer_pair_opts;", text)
    assert "mh_icp_align_layers_opts" in capi._SIGNATURES
    assert hasattr(capi.lib(), "mh_icp_align_layers_opts")
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib()._name], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mh_icp_align_layers_opts$", out, re.M)
    import ctypes as C
    assert C.sizeof(capi.LayerPairOpts) == 4


def test_abi_version_is_still_7():
    assert capi.lib().mh_abi_version() == 7


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


def _path(hl, text):
    icp, _ = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(text))
    return icp.alignPath()


def _unique(text):
    assert "allowMatchAlreadyMatchedGlobalPoints: true" in text
    return text.replace("allowMatchAlreadyMatchedGlobalPoints: true", "allowMatchAlreadyMatchedGlobalPoints: false")


ONE = _HEAD + _points("2.0*ADAPTIVE_THRESHOLD_SIGMA", [("localmap", "decimated_for_icp", 1.0)]) + _TAIL
TWO = _HEAD + _points("3.0*ADAPTIVE_THRESHOLD_SIGMA", [("localmap", "decimated_for_icp", 1.0)]) + \
    _points("2.0*ADAPTIVE_THRESHOLD_SIGMA", [("localmap_far", "decimated_for_icp_near", 1.0)]) + _TAIL


def test_one_unique_matcher_takes_the_layers_path(hl):
    """The single-pair chains do not implement the claims: the one-matcher pipeline that writes `false` runs on the multi-layer
    loop (mh_icp_align_layers_opts, one pair), the same pipeline with `true` stays where it was."""
    assert _path(hl, _unique(ONE)) == "layers"
    assert _path(hl, ONE) == "single"


def test_two_unique_matchers_take_the_layers_path(hl):
    assert _path(hl, _unique(TWO)) == "layers"
    assert _path(hl, TWO) == "layers"


def test_unique_shapes_the_fused_loop_does_not_take(hl):
    """pairingsPerPoint 2, an iteration gate, more than MH_MAX_LAYER_PAIRS entries: the matcher-by-matcher loop, which applies
    the claims on the host; forceGenericPath likewise."""
    two_per_point = _HEAD + _points("2.0", [("a", "x", 1.0)], ppp=2) + _TAIL
    gated = _HEAD + _points("2.0", [("a", "x", 1.0)], run_from=4) + _TAIL
    nine = _HEAD + _points("2.0", [(f"g{i}", f"l{i}", 1.0) for i in range(9)]) + _TAIL
    for text in (two_per_point, gated, nine):
        assert _path(hl, _unique(text)) == "generic"
    icp, _ = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(_unique(ONE)))
    icp.forceGenericPath(True)
    assert icp.alignPath() == "generic"


def test_the_parallel_form_is_the_serial_walk(oracle, small_workload):
    """What the device computes -- the winner of map point g is the smallest (pair order << 29 | local index) among the unique
    pairs' candidates naming g -- against the serial walk of unique_global_ref.ClaimMatcher, on the CPU oracle's candidates of
    two pairs sharing one map (flags [1, 1], [1, 0], [0, 1]) at the small workload's initial guess."""
    import numpy as np
    from unique_global_ref import ClaimMatcher
    w = small_workload
    om = oracle.Map(w.voxel_size, w.cap).insert(w.map_xyz)
    locs = [np.ascontiguousarray(w.scan_xyz[0::2]), np.ascontiguousarray(w.scan_xyz[1::2])]
    thr = [4.0 * w.sigma, 3.0 * w.sigma + 0.2]
    cands = [oracle.match_points(om, l, w.T_guess, t, 0.0) for l, t in zip(locs, thr)]
    assert all(len(c["local_idx"]) > 100 for c in cands)
    for flags in ([1, 1], [1, 0], [0, 1]):
        serial = ClaimMatcher(flags)
        want = [serial(om, l, w.T_guess, t, 0.0) for l, t in zip(locs, thr)]
        table = {}
        for i, c in enumerate(cands):
            if flags[i]:
                for li, g in zip(c["local_idx"].tolist(), c["global_idx"].tolist()):
                    table[g] = min(table.get(g, 1 << 62), (i << 29) | li)
        for i, c in enumerate(cands):
            keep = np.array([not flags[i] or table[g] == ((i << 29) | li)
                             for li, g in zip(c["local_idx"].tolist(), c["global_idx"].tolist())], bool)
            np.testing.assert_array_equal(c["local_idx"][keep], want[i]["local_idx"])
            np.testing.assert_array_equal(c["global_idx"][keep], want[i]["global_idx"])
        assert serial.dropped > 0
