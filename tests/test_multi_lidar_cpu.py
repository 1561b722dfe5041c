"""Multi-LiDAR rigs without a device: the numpy restatement of mh_scan_merge_sensors (tests/merge_ref.py) against hand-worked
cases and the oracle's time-stamp adjustment, the binding's struct against the header, the exported symbol, the grouping
rule (SensorSync), and initialize() reading params.multiple_lidars / params.lidar_sensor_labels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

import merge_ref as MR
import multi_lidar_inline as ML
import rgbd_inline as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mh_scan_merge_sensors"
F = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def test_a_quarter_turn_and_a_shift_on_representable_points():
    P = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])  # 90 deg about z, then a shift
    p = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.5], [-4.0, 8.0, -16.0]], F)
    want = np.array([[1.0, 3.0, 3.0], [-1.0, 2.0, 3.5], [-7.0, -2.0, -13.0]], F)
    got = MR.transform(P, p)
    assert got.dtype == F and np.array_equal(got, want)
    assert np.array_equal(MR.transform(np.eye(4)[:3], p), p)


def test_middle_and_earliest_by_hand():
    t = np.array([-0.03, 0.01, 0.05], F)
    tmin, tmax = F(-0.03), F(0.05)
    mid = F(0.5) * (tmin + tmax)
    assert np.array_equal(MR.adjust(t, MR.TS_MIDDLE_IS_ZERO, 0.0), (t - mid) + F(0.0))
    assert np.array_equal(MR.adjust(t, MR.TS_EARLIEST_IS_ZERO, 0.25), (t - tmin) + F(0.25))
    assert MR.adjust(t, MR.TS_EARLIEST_IS_ZERO, 0.0)[0] == 0.0 and abs(MR.adjust(t, MR.TS_MIDDLE_IS_ZERO, 0.0)[1]) < 1e-8
    assert np.array_equal(MR.adjust(t, MR.TS_NONE, 7.0), t)
    assert MR.tmin_tmax(np.array([0.0, -0.0], F))[0].view(np.uint32) == 0x80000000  # -0 is the smaller one


def test_time_part_equals_the_oracle_source_by_source(oracle):
    rng = np.random.default_rng(11)
    srcs = []
    for n, method, off in ((257, MR.TS_MIDDLE_IS_ZERO, 0.004), (64, MR.TS_EARLIEST_IS_ZERO, -0.0125), (5, MR.TS_NONE, 0.3),
                           (1000, MR.TS_MIDDLE_IS_ZERO, 0.0)):
        t = rng.uniform(-0.06, 0.05, n).astype(F)
        srcs.append(dict(xyz=rng.normal(size=(n, 3)).astype(F), t=t, method=method, offset=off))
    got = MR.merge(srcs)
    want = np.concatenate([s["t"] if s["method"] == MR.TS_NONE else oracle.adjust_timestamps(s["t"], s["method"], s["offset"])
                           for s in srcs])
    assert np.array_equal(got["t"].view(np.uint32), want.view(np.uint32))
    assert got["i"] is None and len(got["xyz"]) == 257 + 64 + 5 + 1000


def test_merge_appends_in_order_and_skips_empty_sources():
    a = dict(xyz=np.ones((2, 3), F), t=None, i=np.array([1, 2], F))
    e = dict(xyz=np.zeros((0, 3), F), t=None, i=None)
    b = dict(xyz=2 * np.ones((1, 3), F), t=None, i=np.array([3], F), pose=np.array([[1, 0, 0, 10.0], [0, 1, 0, 0], [0, 0, 1, 0]]))
    m = MR.merge([a, e, b])
    assert m["t"] is None and list(m["i"]) == [1, 2, 3] and np.array_equal(m["xyz"][:, 0], np.array([1, 1, 12], F))
    with pytest.raises(AssertionError):
        MR.merge([a, dict(xyz=np.ones((1, 3), F), t=None, i=None)])


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbol_is_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "mola_lidar_odometry_amd", "libmolahip.so")],
                                  text=True)
    assert re.search(r"\bT %s$" % NAME, out, re.M)
    assert re.search(r"\bT mh_scan_deskew$", out, re.M)  # (the entry points before it stay)
    assert NAME in capi._SIGNATURES and hasattr(capi.lib(), NAME)


def test_merge_source_layout_matches_c(tmp_path):
    fields = [f for f, _ in capi.MergeSource._fields_]
    prog = tmp_path / "ms.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "molahip.h"\nint main(void){\n'
                    '  printf("%zu %d %d", sizeof(mh_merge_source), MH_ABI_VERSION, MH_MAX_MERGE_SOURCES);\n' +
                    "".join('  printf(" %%zu", offsetof(mh_merge_source, %s));\n' % f for f in fields) + "  return 0; }\n")
    exe = tmp_path / "ms"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.MergeSource
    assert vals[0] == C.sizeof(S) == 104
    assert vals[1] == 7 == int(capi.lib().mh_abi_version())
    assert vals[2] == capi.MAX_MERGE_SOURCES == 8
    assert vals[3:] == [getattr(S, f).offset for f in fields] == [0, 96, 100]
    assert fields == ["sensor_pose", "timestamp_method", "time_offset"]
    m = capi.merge_source()
    assert list(m.sensor_pose) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and (m.timestamp_method, m.time_offset) == (0, 0.0)
    m = capi.merge_source(np.arange(12.0).reshape(3, 4), capi.TS_EARLIEST_IS_ZERO, 0.5)
    assert list(m.sensor_pose) == list(range(12)) and (m.timestamp_method, m.time_offset) == (2, 0.5)


# ------------------------------------------------------------------------------------------------ the grouping rule
@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def test_sync_waits_until_all_labels_are_present(host):
    s = host.SensorSync(3, 0.01)
    assert s.push("b", 1.000) is None and s.push("a", 1.001) is None and s.waiting() == ["a", "b"]
    labels, dts, discarded = s.push("c", 1.002)
    assert labels == ["a", "b", "c"] and discarded == [] and s.waiting() == []
    assert dts == [0.0, 1.000 - 1.001, 1.002 - 1.001]
    assert s.push("a", 2.0) is None  # and the next group starts empty


def test_sync_label_order_beats_arrival_order(host):
    s = host.SensorSync(2, 0.01)
    assert s.push("rear", 5.004) is None
    labels, dts, discarded = s.push("front", 5.000)  # front arrives last, and is the reference all the same
    assert labels == ["front", "rear"] and dts == [0.0, 5.004 - 5.000] and discarded == []
    assert s.push("front", 5.100) is None
    labels, dts, _ = s.push("rear", 5.104)
    assert labels == ["front", "rear"] and dts == [0.0, 5.104 - 5.100]


def test_sync_discards_what_is_outside_the_window(host):
    s = host.SensorSync(3, 0.01)
    s.push("a", 1.000)          # 50 ms before the trigger: out
    s.push("b", 1.045)
    labels, dts, discarded = s.push("c", 1.050)
    assert labels == ["b", "c"] and discarded == ["a"] and s.waiting() == []
    assert dts == [0.0, 1.050 - 1.045]  # relative to the first KEPT observation
    s = host.SensorSync(2, 0.01)
    s.push("a", 1.0)
    assert s.push("b", 1.010 + 1e-9)[0] == ["b"]  # just outside; the trigger itself always stays
    s.push("a", 2.0)
    assert s.push("b", 2.0 + 0.0099)[0] == ["a", "b"]


def test_sync_newer_observation_replaces_the_older_one(host):
    s = host.SensorSync(2, 0.01)
    assert s.push("a", 1.00) is None and s.push("a", 1.10) is None and s.waiting() == ["a"]
    labels, dts, discarded = s.push("b", 1.104)
    assert labels == ["a", "b"] and discarded == [] and abs(dts[1] - 0.004) < 1e-12  # the 1.10 one: 1.00 would be out
    one = host.SensorSync(1, 0.01)
    assert one.push("x", 3.0) == (["x"], [0.0], []) and one.waiting() == []


# ------------------------------------------------------------------------------------------------ initialize()
def test_initialize_reads_the_two_parameter_groups(host):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(ML.pipeline(2, 0.0125, [ML.FRONT, "rear_.*"])))
    d = lo.describePipeline()
    assert d["multiple_lidars"] == "lidar_count 2 max_time_offset 0.0125"
    assert d["lidar_sensor_labels"] == "%s | rear_.*" % ML.FRONT
    assert d["layer_for_icp"] == "decimated_for_icp"  # still the default chain
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(ML.pipeline(1, 0.1, "lidar")))  # a scalar
    assert lo.describePipeline()["lidar_sensor_labels"] == "lidar"
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")))  # neither group
    d = lo.describePipeline()
    assert d["multiple_lidars"] == "lidar_count 1 max_time_offset 0.025" and d["lidar_sensor_labels"] == "(any)"
    assert "observations_filter_adjust_timestamps" not in ML.pipeline(2, adjust_timestamps=False)
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(ML.pipeline(2, adjust_timestamps=False)))
    assert lo.describePipeline()["timestamp_method"] == "0"


def test_initialize_refuses_what_the_device_does_not_merge(host):
    with pytest.raises(RuntimeError, match="lidar_count is 9"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(ML.pipeline(9)))
    host.LidarOdometry().initialize(host.Config.FromYamlText(ML.pipeline(8)))
    text = RG.pipeline()
    assert text.startswith("params:\n")
    rig = text.replace("params:\n", "params:\n  multiple_lidars:\n    lidar_count: 2\n    max_time_offset: 0.01\n", 1)
    with pytest.raises(RuntimeError, match="depth"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(rig))
    one = text.replace("params:\n", "params:\n  multiple_lidars:\n    lidar_count: 1\n", 1)
    host.LidarOdometry().initialize(host.Config.FromYamlText(one))
    with pytest.raises(RuntimeError, match="regular expression"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(ML.pipeline(2, labels="lidar_(")))


def test_a_rig_refuses_unlabelled_observations_before_any_device_work(host):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(ML.pipeline(2)))
    xyz = np.zeros((10, 3), F)
    with pytest.raises(RuntimeError, match="onLidarFrom"):
        lo.onLidar(0.0, xyz)
    with pytest.raises(RuntimeError, match="onLidarFrom"):
        lo.prefetch(xyz)
    assert lo.records() == []
    r = lo.onLidarFrom("camera", 0.0, xyz)  # not a LiDAR of ours: ignored before anything touches a device
    assert r["ignored"] and not r["waiting"] and not r["dropped"] and r["n_sensors"] == 0 and len(lo.records()) == 1
