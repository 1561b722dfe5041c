"""The range-image generator without a device: the numpy restatement (tests/rimg_ref.py) against hand-worked cases, the
binding's struct against the header, the exported symbol, and the rgbd-shaped pipeline (tests/rgbd_inline.py) loading into a
depth-image plan that refuses point clouds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

import rgbd_inline as RG
import rimg_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mh_scan_edges_from_range_image"


@pytest.mark.parametrize("W", [1, 6, 64])
def test_a_linear_ramp_scores_zero_everywhere(W):
    cols = 2 * W + 40
    R = (1000 + 7 * np.arange(cols, dtype=np.int64))[None, :].repeat(3, 0).astype(np.uint16)
    scored, S = RR.scores(R, W)
    assert scored[:, W:cols - W].all() and not scored[:, :W].any() and not scored[:, cols - W:].any()
    assert (S == 0).all()
    edge, plane = RR.classify(R, W, 0.0)  # (0 > 0 is false: all planes)
    assert not edge.any() and plane.sum() == 3 * (cols - 2 * W)


def test_a_step_scores_the_hand_value():
    W = 2
    R = np.array([[100] * 6 + [160] * 6], np.uint16)  # a step of 60 between columns 5 and 6
    scored, S = RR.scores(R, W)
    # window of 5: column 4 sees one high sample (+60), column 5 two (+120); column 6 two low ones (-120), column 7 one (-60)
    assert list(S[0]) == [0, 0, 0, 0, 60, 120, -120, -60, 0, 0, 0, 0]
    assert list(scored[0]) == [False] * 2 + [True] * 8 + [False] * 2
    edge, plane = RR.classify(R, W, 60.0)  # strict: |S| = 60 stays a plane
    assert list(np.nonzero(edge[0])[0]) == [5, 6] and list(np.nonzero(plane[0])[0]) == [2, 3, 4, 7, 8, 9]


@pytest.mark.parametrize("W", [1, 6])
def test_a_zero_unscores_exactly_its_window(W):
    cols = 6 * W + 5
    R = np.full((2, cols), 1234, np.uint16)
    z = 3 * W + 1
    R[1, z] = 0
    scored, _ = RR.scores(R, W)
    assert scored[0, W:cols - W].all()
    want = np.ones(cols, bool)
    want[:W] = want[cols - W:] = False
    want[z - W:z + W + 1] = False  # the 2W + 1 pixels around it
    assert np.array_equal(scored[1], want) and (~want[W:cols - W]).sum() == 2 * W + 1


def test_points_follow_the_written_operations():
    R = np.array([[0, 0, 0], [0, 2000, 0], [0, 0, 0]], np.uint16)
    m = R > 0
    P = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])  # 90 deg about z, then a shift
    p = RR.points(R, m, 2.0, 4.0, 2.0, 3.0, 0.001, True, P)  # d = 2, kx = (2 - 1) / 2 = 0.5, ky = (3 - 1) / 4 = 0.5
    assert p.dtype == np.float32 and np.array_equal(p, np.array([[1.0 - 1.0, 2.0 + 2.0, 3.0 + 1.0]], np.float32))
    q = RR.points(R, m, 2.0, 4.0, 2.0, 3.0, 0.001, False, np.eye(4)[:3])  # along the ray: xs = 2 / sqrt(1.5)
    xs = np.float32(2.0 / np.sqrt(1.5))
    assert np.array_equal(q, np.array([[xs, xs * np.float32(0.5), xs * np.float32(0.5)]], np.float32))


def test_symbol_is_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "mola_lidar_odometry_amd", "libmolahip.so")],
                                  text=True)
    assert re.search(r"\bT %s$" % NAME, out, re.M)
    assert re.search(r"\bT mh_scan_curvature$", out, re.M)  # (the entry points before it stay)
    assert NAME in capi._SIGNATURES and hasattr(capi.lib(), NAME)


def test_range_image_params_layout_matches_c(tmp_path):
    fields = [f for f, _ in capi.RangeImageParams._fields_]
    prog = tmp_path / "rip.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "molahip.h"\nint main(void){\n'
                    '  printf("%zu %d", sizeof(mh_range_image_params), MH_ABI_VERSION);\n' +
                    "".join('  printf(" %%zu", offsetof(mh_range_image_params, %s));\n' % f for f in fields) + "  return 0; }\n")
    exe = tmp_path / "rip"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.RangeImageParams
    assert vals[0] == C.sizeof(S) == 136
    assert vals[1] == 7 == int(capi.lib().mh_abi_version())
    assert vals[2:] == [getattr(S, f).offset for f in fields]
    assert fields == ["rows", "cols", "fx", "fy", "cx", "cy", "range_units", "range_is_depth", "sensor_pose",
                      "row_window_length", "score_threshold"]
    p = capi.range_image_params(120, 160, 140.0, 141.0, 79.5, 59.5)
    assert (p.row_window_length, p.score_threshold, p.range_is_depth) == (6, 10.0, 1) and list(p.sensor_pose)[::5] == [1.0, 1.0, 1.0]


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def test_rgbd_text_loads_into_a_depth_image_plan(host):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(RG.pipeline()))
    d = lo.describePipeline()
    assert d["plan"] == "general" and d["input"] == "depth_image"
    assert d["step:00"].startswith("pass0 GeneratorEdgesFromRangeImage depth image -> edges,planes (row_window_length 6)")
    assert int(d["steps"]) == 6 and all(d[f"step:{k:02d}"].startswith("pass1 ") for k in range(1, 6))
    assert d["map:localmap_edges"].endswith("HashedVoxelPointCloud") and d["map:localmap_planes"].endswith("SparseTreesPointCloud")
    assert d["merge:edges_for_map"] == "localmap_edges" and d["merge:planes_for_map"] == "localmap_planes"
    assert d["icp_path"] == "layers"
    assert lo.localMapClasses() == {"localmap_edges": "", "localmap_planes": ""}  # created at the first key-frame
    for planes_map in (RG.HASHED_PLANES.format(cap=0), RG.HASHED_PLANES.format(cap=20)):  # the variants load as well
        lo2 = host.LidarOdometry()
        lo2.initialize(host.Config.FromYamlText(RG.pipeline(planes_map)))
        assert lo2.describePipeline()["map:localmap_planes"].endswith("HashedVoxelPointCloud")


def test_wrong_input_for_the_plan_throws(host):
    import lidar2d_inline as L2
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(RG.pipeline()))
    with pytest.raises(RuntimeError, match="onDepthImage"):
        lo.onLidar(0.0, np.zeros((10, 3), np.float32))
    assert lo.records() == []
    cloud = host.LidarOdometry()
    cloud.initialize(host.Config.FromYamlText(L2.pipeline()))
    with pytest.raises(RuntimeError, match="onDepthImage"):
        cloud.onDepthImage(0.0, np.zeros((RG.ROWS, RG.COLS), np.uint16), RG.FX, RG.FY, RG.CX, RG.CY)
    with pytest.raises(RuntimeError, match="uint16"):
        lo.onDepthImage(0.0, np.zeros((RG.ROWS, RG.COLS), np.float32), RG.FX, RG.FY, RG.CX, RG.CY)


def test_other_generators_and_a_layer_named_raw_are_refused(host):
    text = RG.pipeline().replace("GeneratorEdgesFromRangeImage", "GeneratorSomethingElse")
    with pytest.raises(RuntimeError, match="GeneratorSomethingElse"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(text))
    text = RG.pipeline().replace("target_layer: 'edges'", "target_layer: 'raw'")
    with pytest.raises(RuntimeError, match="unsupported observation filter chain"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(text))


def test_renderer_shows_the_room(host):
    img = RG.render(np.eye(4))
    assert img.shape == (RG.ROWS, RG.COLS) and img.dtype == np.uint16
    assert img[RG.ROWS // 2, RG.COLS // 2] in (5899, 5900, 5901)  # the far wall at x = 6 from the camera at x = 0.1
    edge, plane = RR.classify(img, RG.W, RG.SCORE_THRESHOLD)
    assert edge.sum() > 300 and plane.sum() > 8000
