"""Stand-alone driver on filter chains other than the default one (general plans over named device layers): the reference's
extras pipelines and inline equivalents are recognised and described (CPU), intensity filters are rejected (CPU), and on the
GPU the edges-, dual-map- and near-far-shaped chains track a synthetic drive, deterministically and identically through
onLidar and the interleaved entry, with observation layers of the sizes a numpy restatement of the chain gives."""
import os

import numpy as np
import pytest

from mola_lidar_odometry_amd import synth, trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
REF_EXTRAS = "/root/reference/pipelines/extras"

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


_FRONT = f"""  - class_name: mp2p_icp_filters::FilterDeskew
    params:
      input_pointcloud_layer: 'raw'
      output_pointcloud_layer: 'deskewed'
      silently_ignore_no_timestamps: true
      twist: [vx,vy,vz,wx,wy,wz]
  - class_name: mp2p_icp_filters::FilterByRange
    params:
      input_pointcloud_layer: 'deskewed'
      output_layer_between: 'range_filtered'
      range_min: max(1.0, 0.05*{_E})
      range_max: 1.2*{_E}
  - class_name: mp2p_icp_filters::FilterBoundingBox
    params:
      input_pointcloud_layer: 'range_filtered'
      outside_pointcloud_layer: 'filtered'
      bounding_box_min: [ -0.30*{_E}, -0.30*{_E}, 0.05*{_E} ]
      bounding_box_max: [  0.30*{_E},  0.30*{_E}, 0.40*{_E} ]
"""

# the structure and values of extras/lidar3d-edges.yaml
EDGES_TAIL = ("localmap_generator:\n" + _map("localmap_small_curvature", 20) + _map("localmap_large_curvature", 10) +
              "observations_filter_1st_pass:\n" + _FRONT + """  - class_name: mp2p_icp_filters::FilterCurvature
    params:
      input_pointcloud_layer: 'filtered'
      output_layer_larger_curvature: 'large_curvature'
      output_layer_smaller_curvature: 'smaller_curvature'
      max_cosine: 0.4
      min_clearance: 0.20
      max_gap: 1.0
""" + _decimate("large_curvature", "decimated_for_map_large_curvature", f"1.0*1e-2*{_E}") +
              _decimate("decimated_for_map_large_curvature", "decimated_for_icp_large_curvature", f"1.5*1e-2*{_E}") +
              _decimate("smaller_curvature", "decimated_for_map_smaller_curvature", f"0.5*1e-2*{_E}") +
              _decimate("decimated_for_map_smaller_curvature", "decimated_for_icp_smaller_curvature", f"2.0*1e-2*{_E}") +
              """  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['raw', 'deskewed', 'filtered', 'range_filtered', 'large_curvature', 'smaller_curvature']
insert_observation_into_local_map:
""" + _merge("decimated_for_map_smaller_curvature", "localmap_small_curvature") +
              _merge("decimated_for_map_large_curvature", "localmap_large_curvature"))
EDGES_MATCHES = ('          - {global: "localmap_large_curvature", local: "decimated_for_icp_large_curvature", weight: 1.0}\n'
                 '          - {global: "localmap_small_curvature", local: "decimated_for_icp_smaller_curvature", weight: 1.0}\n')

# the structure and values of extras/lidar3d-dual-map.yaml
DUAL_TAIL = ("localmap_generator:\n" + _map("localmap", 20) + _map("localmap_far", 10, "1.10") +
             "observations_filter_1st_pass:\n" + _FRONT + f"""  - class_name: mp2p_icp_filters::FilterBoundingBox
    params:
      input_pointcloud_layer: 'filtered'
      inside_pointcloud_layer: 'near'
      outside_pointcloud_layer: 'far'
      bounding_box_min: [ -0.30*{_E}, -0.30*{_E}, -1000.0 ]
      bounding_box_max: [  0.30*{_E},  0.30*{_E}, -1.0 ]
""" + _decimate("near", "decimated_for_icp_near", f"2.00*1e-2*{_E}") +
             _decimate("far", "decimated_for_map_far", f"1.00*1e-2*{_E}") +
             _decimate("filtered", "decimated_for_icp", f"1.50*1e-2*{_E}") +
             _decimate("range_filtered", "decimated_for_map", f"0.5*1e-2*{_E}") +
             """  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['raw', 'deskewed', 'range_filtered', 'filtered', 'far', 'near']
insert_observation_into_local_map:
""" + _merge("decimated_for_map", "localmap") + _merge("decimated_for_map_far", "localmap_far"))
DUAL_MATCHES = ('          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}\n'
                '          - {global: "localmap_far", local: "decimated_for_map_far", weight: 0.5}\n')

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
NEARFAR_MATCHES = ('          - {global: "localmap_near", local: "decimated_for_icp_near", weight: 1.0}\n'
                   '          - {global: "localmap_far", local: "decimated_for_icp_far", weight: 1.0}\n')


def inline_pipeline(tail, matches):
    """The repo's default pipeline with its ICP layer pairs and everything from localmap_generator on replaced."""
    head = open(PIPE).read().split("\nlocalmap_generator:")[0] + "\n"
    one = '          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}\n'
    assert one in head
    return head.replace(one, matches) + tail


CHAINS = {"edges": (EDGES_TAIL, EDGES_MATCHES), "dual-map": (DUAL_TAIL, DUAL_MATCHES), "near-far": (NEARFAR_TAIL, NEARFAR_MATCHES)}


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _load(host, text):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(text))
    return lo


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["lidar3d-edges.yaml", "lidar3d-dual-map.yaml", "lidar3d-kissicp-like.yaml"])
def test_driver_recognises_reference_extras(host, name):
    path = os.path.join(REF_EXTRAS, name)
    if not os.path.exists(path):
        pytest.skip("reference tree not present on this box")
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(path))
    d = lo.describePipeline()
    assert d["plan"] == "general" and int(d["steps"]) >= 4
    maps = sorted(k[4:] for k in d if k.startswith("map:"))
    want = {"lidar3d-edges.yaml": ["localmap_large_curvature", "localmap_small_curvature"],
            "lidar3d-dual-map.yaml": ["localmap", "localmap_far"], "lidar3d-kissicp-like.yaml": ["localmap"]}[name]
    assert maps == want
    if name == "lidar3d-edges.yaml":
        steps = [d[f"step:{i:02d}"] for i in range(int(d["steps"]))]
        assert "pass1 FilterCurvature filtered -> large_curvature,smaller_curvature,-" in steps
        assert d["merge:decimated_for_map_large_curvature"] == "localmap_large_curvature"


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_driver_recognises_inline_chains(host, chain):
    d = _load(host, inline_pipeline(*CHAINS[chain])).describePipeline()
    assert d["plan"] == "general"
    assert d["icp_path"] == "layers"  # (two point-layer pairs in every inline chain)
    steps = [d[f"step:{i:02d}"] for i in range(int(d["steps"]))]
    if chain == "edges":
        assert steps[0] == "pass1 FilterDeskew raw -> deskewed"
        assert steps[2] == "pass1 FilterBoundingBox range_filtered -> filtered (outside)"
        assert steps[3] == "pass1 FilterCurvature filtered -> large_curvature,smaller_curvature,-"
        assert sorted(k for k in d if k.startswith("map:")) == ["map:localmap_large_curvature", "map:localmap_small_curvature"]
    if chain == "dual-map":  # a box with both outputs is two steps
        assert "pass1 FilterBoundingBox filtered -> near (inside)" in steps
        assert "pass1 FilterBoundingBox filtered -> far (outside)" in steps
    if chain == "near-far":
        assert int(d["timestamp_method"]) == 1
        assert "pass2 FilterDeskew decimated_for_icp_near_skewed -> decimated_for_icp_near" in steps


def test_default_chain_keeps_its_plan(host):
    d = _load(host, open(PIPE).read()).describePipeline()
    assert "plan" not in d and d["layer_for_icp"] == "decimated_for_icp"


def test_intensity_filters_are_rejected(host, tmp_path):
    text = inline_pipeline(*CHAINS["edges"]).replace("""  - class_name: mp2p_icp_filters::FilterCurvature""", """  - class_name: mp2p_icp_filters::FilterNormalizeIntensity
    params:
      pointcloud_layer: 'filtered'
  - class_name: mp2p_icp_filters::FilterCurvature""")
    with pytest.raises(RuntimeError, match="unsupported observation filter chain.*FilterNormalizeIntensity"):
        _load(host, text)
    text = inline_pipeline(*CHAINS["edges"]).replace("FilterCurvature", "FilterByIntensity")
    with pytest.raises(RuntimeError, match="unsupported observation filter chain.*FilterByIntensity"):
        _load(host, text)
    path = os.path.join(REF_EXTRAS, "lidar3d-intensity.yaml")
    if os.path.exists(path):
        with pytest.raises(RuntimeError, match="unsupported observation filter chain.*Intensity"):
            host.LidarOdometry().initialize(host.Config.FromYamlFile(path))


def test_chain_errors_name_the_problem(host):
    bad = inline_pipeline(*CHAINS["edges"]).replace("input_pointcloud_layer: 'large_curvature'", "input_pointcloud_layer: 'nowhere'")
    with pytest.raises(RuntimeError, match="unsupported observation filter chain.*'nowhere'"):
        _load(host, bad)
    bad = inline_pipeline(*CHAINS["edges"]).replace("target_layer: 'localmap_large_curvature'\n      input", "target_layer: 'nomap'\n      input")
    with pytest.raises(RuntimeError, match="unsupported observation filter chain.*'nomap'"):
        _load(host, bad)


# ------------------------------------------------------------------------------------------------ GPU
def _ate(recs, drive):
    G = np.stack([trajectory.to44(p) for p in drive["poses"]])
    G = np.linalg.inv(G[0])[None] @ G
    E = np.stack([trajectory.to44(r["pose"]) for r in recs])
    return float(np.sqrt(np.mean(np.sum((E[:, :3, 3] - G[:len(E), :3, 3]) ** 2, 1))))


def _run(host, text, drive, interleaved=False, profile=None):
    lo = host.LidarOdometry(0, True)
    lo.initialize(host.Config.FromYamlText(text))
    for k, (xyz, t) in enumerate(drive["scans"]):
        if interleaved:
            rec = np.concatenate([xyz, t[:, None]], 1).astype(np.float32)
            lo.onLidar(float(drive["stamps"][k]), rec, None, [0, 1, 2], 3)
        else:
            lo.onLidar(float(drive["stamps"][k]), xyz, t)
    if profile is not None:
        profile.update(lo.profile())
    return lo.records()


def _comparable(recs):
    return [{k: v for k, v in r.items()} for r in recs]


@pytest.fixture(scope="module")
def drive():
    return synth.make_drive(14)


def _restated_edges_layers(xyz, t, twist, R):
    """The edges chain in numpy / the CPU oracle for one scan: sensor range estimate R, de-skew twist."""
    from oracle import oracle_c
    import importlib.util
    spec = importlib.util.spec_from_file_location("_curv", os.path.join(ROOT, "tests", "test_curvature.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    d = oracle_c.deskew(xyz, t, np.asarray(twist, np.float64))
    rmin, rmax = max(1.0, 0.05 * R), 1.2 * R
    k1 = oracle_c.filter_by_range(d, rmin, rmax)
    box = [(-0.30 * R, -0.30 * R, 0.05 * R), (0.30 * R, 0.30 * R, 0.40 * R)]
    k2 = k1[oracle_c.filter_bbox(d[k1], box[0], box[1], keep_inside=False)]
    f = d[k2]
    cls = cm.curvature_classes(f)
    out = {}
    for name, c, r1, r2 in (("large_curvature", 0, 1.0e-2, 1.5e-2), ("smaller_curvature", 1, 0.5e-2, 2.0e-2)):
        lay = f[cls == c]
        i1 = oracle_c.decimate_first_point(lay, r1 * R)
        i2 = oracle_c.decimate_first_point(lay[i1], r2 * R)
        out["decimated_for_map_" + name] = len(i1)
        out["decimated_for_icp_" + name] = len(i2)
    return out


@pytest.mark.gpu
def test_edges_chain_tracks_the_drive(host, drive):
    text = inline_pipeline(*CHAINS["edges"])
    prof = {}
    recs = _run(host, text, drive, profile=prof)
    assert not any(r["dropped"] for r in recs)
    # the first scan: no motion yet (twist 0), the sensor range from the raw cloud -- the chain restated layer by layer
    xyz, t = drive["scans"][0]
    mn, mx = xyz.min(0), xyz.max(0)
    R0 = max(float(max(np.float32(np.sqrt((mx * mx).sum(dtype=np.float32))), np.float32(np.sqrt((mn * mn).sum(dtype=np.float32))))), 5.0)
    want = _restated_edges_layers(xyz, t, np.zeros(6), R0)
    assert recs[0]["layer_sizes"] == want, (recs[0]["layer_sizes"], want)
    for r in recs[2:]:
        assert r["icp_run"] and r["icp_good"], r
    assert prof.get("icp.align_calls", 0) > 0
    ate = _ate(recs, drive)
    print(f"edges chain: ATE RMSE {ate:.4f} m over {len(recs)} scans")
    # (tests/test_odometry.py holds the default chain to 0.2 m on this drive; the edges chain measured 0.32 m: the curvature split
    # of these 600-azimuth sweeps keeps points of 19 m to 95 m range only -- the neighbour spacing, ~0.0105 x range, must lie
    # between min_clearance 0.2 m and max_gap 1.0 m -- so fewer, farther points constrain the pose)
    assert ate < 0.5, ate
    # deterministic, and the same through the interleaved entry
    again = _run(host, text, drive)
    assert _comparable(again) == _comparable(recs)
    inter = _run(host, text, drive, interleaved=True)
    assert _comparable(inter) == _comparable(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["dual-map", "near-far"])
def test_other_chains_track_the_drive(host, drive, chain):
    text = inline_pipeline(*CHAINS[chain])
    recs = _run(host, text, drive)
    assert not any(r["dropped"] for r in recs)
    for r in recs[2:]:
        assert r["icp_run"] and r["icp_good"], r
    print(f"{chain} chain: ATE RMSE {_ate(recs, drive):.4f} m")
    assert _ate(recs, drive) < 0.2  # (measured: dual-map 0.075 m, near-far 0.105 m)
    assert _comparable(_run(host, text, drive)) == _comparable(recs)
    assert _comparable(_run(host, text, drive, interleaved=True)) == _comparable(recs)


@pytest.mark.gpu
def test_edges_chain_takes_the_fused_layers_route(host, drive):
    """Two (map, scan) pairs of one matcher: every alignment runs on mh_icp_align_layers."""
    text = inline_pipeline(*CHAINS["edges"])
    prof = {}
    recs = _run(host, text, drive, profile=prof)
    runs = sum(1 for r in recs if r["icp_run"])
    assert runs == len(recs) - 1 and prof["icp.align_calls"] >= runs
    assert prof["icp.fused_align_calls"] == prof["icp.align_calls"]
