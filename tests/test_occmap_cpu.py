"""The occupancy voxel map (mrpt::maps::CVoxelMap stand-in) without a device: the closed form of the line walk against the
sequential walk, hand-computed known answers of the restatement, the C ABI's layouts and refusals, and the driver's
initialisation on the lidar2d-shaped pipeline."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

import lidar2d_inline
import occmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIDAR2D = "/root/reference/pipelines/lidar2d.yaml"


# ------------------------------------------------------------------------------------------------ the walk
def test_closed_form_equals_sequential_walk_on_random_rays():
    rng = np.random.default_rng(1)
    for _ in range(1500):
        o = rng.integers(-50, 50, 3)
        e = o + rng.integers(-400, 400, 3) * rng.integers(0, 2, 3)
        assert R.walk_closed_form(o, e) == R.walk_sequential(o, e)
    for _ in range(60):  # long ones, far from zero
        o = rng.integers(-900000, 900000, 3)
        e = o + rng.integers(-3000, 3000, 3)
        assert R.walk_closed_form(o, e) == R.walk_sequential(o, e)


@pytest.mark.parametrize("d", [(9, 0, 0), (0, -9, 0), (0, 0, 9), (7, 7, 7), (-7, 7, -7), (6, -6, 0), (0, 5, 5),
                               (8, 4, 0), (-8, 0, 4), (4, -8, 0), (2, 1, 0), (20, 10, 0), (0, 2, -1)])
def test_closed_form_on_axis_diagonal_and_two_to_one_rays(d):
    for o in ((0, 0, 0), (-3, 11, 5)):
        e = tuple(o[a] + d[a] for a in range(3))
        w = R.walk_sequential(o, e)
        assert R.walk_closed_form(o, e) == w and len(w) == max(abs(v) for v in d) - 1
        assert o not in w and e not in w
        nz = [a for a in range(3) if d[a]]
        if all(abs(d[a]) == abs(d[nz[0]]) for a in nz):  # axis-aligned and exact diagonals: the obvious cells
            assert w == [tuple(o[a] + (d[a] > 0) * k - (d[a] < 0) * k for a in range(3)) for k in range(1, abs(d[nz[0]]))]


def test_rays_of_length_0_1_2():
    assert R.walk_sequential((4, 4, 4), (4, 4, 4)) == [] and R.walk_closed_form((4, 4, 4), (4, 4, 4)) == []
    assert R.walk_sequential((4, 4, 4), (5, 4, 3)) == [] and R.walk_closed_form((4, 4, 4), (5, 4, 3)) == []
    assert R.walk_sequential((0, 0, 0), (2, 0, 0)) == [(1, 0, 0)]
    assert R.walk_sequential((0, 0, 0), (2, 1, 0)) == [(1, 1, 0)]   # 2 * 1 >= 2: the minor axis steps at the half
    assert R.walk_sequential((0, 0, 0), (-2, 2, -1)) == [(-1, 1, -1)]
    assert R.walk_closed_form((0, 0, 0), (2, 1, 0)) == [(1, 1, 0)]


# ------------------------------------------------------------------------------------------------ log-odds
def test_five_integers_of_lidar2d():
    assert R.five_integers(0.70, 0.30, 0.05, 0.95, 0.60) == (14, 14, -47, 47, 7)
    assert R.five_integers(0.5, 0.5, 0.4, 0.6, 0.5)[:2] == (1, 1)  # never below one


@pytest.mark.parametrize("rule", [R.COUNTED, R.ONCE])
def test_saturation_at_both_clamps(rule):
    m = R.OccMapRef(resolution=1.0, update_rule=rule)
    I = [1, 0, 0, 0.5, 0, 1, 0, 0.5, 0, 0, 1, 0.5]
    seen = []
    for _ in range(5):
        m.insert([[3.0, 0.0, 0.0]], I)         # end cell (3, 0, 0); (1, 0, 0) and (2, 0, 0) in between
        seen.append((m.cells[(3, 0, 0)], m.cells[(1, 0, 0)]))
    assert seen == [(14, -14), (28, -28), (42, -42), (47, -47), (47, -47)]
    assert (0, 0, 0) not in m.cells and len(m.cells) == 3
    assert m.centres().tolist() == [[3.5, 0.5, 0.5]]
    for _ in range(8):
        m.insert([[5.0, 0.0, 0.0]], I)         # now (3, 0, 0) lies in between
    assert m.cells[(3, 0, 0)] == -47 and m.cells[(5, 0, 0)] == 47
    assert m.centres().tolist() == [[5.5, 0.5, 0.5]]


def test_counted_and_once_differ_on_a_cell_hit_and_crossed():
    I = [1, 0, 0, 0.5, 0, 1, 0, 0.5, 0, 0, 1, 0.5]
    pts = [[2.0, 0, 0], [2.2, 0, 0], [4.0, 0, 0]]  # two hits on (2, 0, 0), one miss from the ray to (4, 0, 0)
    a = R.OccMapRef(resolution=1.0, update_rule=R.COUNTED).insert(pts, I)
    b = R.OccMapRef(resolution=1.0, update_rule=R.ONCE).insert(pts, I)
    assert a.cells[(2, 0, 0)] == 14 and b.cells[(2, 0, 0)] == 14   # 2 * 14 - 14;  + 14 once, the miss ignored
    assert a.cells[(1, 0, 0)] == -42 and b.cells[(1, 0, 0)] == -14  # three misses; once
    assert a.n_keys == 3 + (1 + 1 + 3)


# ------------------------------------------------------------------------------------------------ C ABI
def test_struct_layouts_and_abi_version(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mh_occmap_params), offsetof(mh_occmap_params, ray_trace_free_space),
    offsetof(mh_occmap_params, max_range), offsetof(mh_occmap_params, far_voxel_metric), offsetof(mh_occmap_params, search_voxel_size),
    offsetof(mh_occmap_params, max_keys_per_pass));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mh_occmap_info), offsetof(mh_occmap_info, l_hit), offsetof(mh_occmap_info, l_occ),
    offsetof(mh_occmap_info, search_voxel_size), offsetof(mh_occmap_info, n_left_out), offsetof(mh_occmap_info, n_passes));
  printf("%d %d %d\n", MH_ABI_VERSION, MH_OCC_COUNTED, MH_OCC_ONCE);
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b, c = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    P, I = capi.OccMapParams, capi.OccMapInfo
    assert [int(v) for v in a.split()] == [C.sizeof(P), P.ray_trace_free_space.offset, P.max_range.offset, P.far_voxel_metric.offset,
                                           P.search_voxel_size.offset, P.max_keys_per_pass.offset]
    assert [int(v) for v in b.split()] == [C.sizeof(I), I.l_hit.offset, I.l_occ.offset, I.search_voxel_size.offset,
                                           I.n_left_out.offset, I.n_passes.offset]
    assert [int(v) for v in c.split()] == [7, capi.OCC_COUNTED, capi.OCC_ONCE]
    assert int(capi.lib().mh_abi_version()) == 7


def _params(**kw):
    d = dict(resolution=0.05, prob_hit=0.7, prob_miss=0.3, clamp_min=0.05, clamp_max=0.95, occupied_threshold=0.6,
             ray_trace_free_space=1, decimation=1, max_range=0.0, update_rule=0, index_mode=0, far_voxel_metric=0,
             search_voxel_size=0.0, reserved_=0, max_keys_per_pass=0)
    d.update(kw)
    return capi.OccMapParams(**d)


@pytest.mark.parametrize("kw,word", [(dict(resolution=0.0), "resolution"), (dict(resolution=-1.0), "resolution"),
                                     (dict(prob_hit=0.0), "prob_hit"), (dict(prob_hit=1.0), "prob_hit"), (dict(prob_miss=1.5), "prob_miss"),
                                     (dict(clamp_min=0.0), "clamp_min"), (dict(clamp_max=1.0), "clamp_max"),
                                     (dict(clamp_min=0.6, clamp_max=0.6), "below clamp_max"), (dict(clamp_min=0.7, clamp_max=0.3), "below clamp_max"),
                                     (dict(decimation=0), "decimation"), (dict(update_rule=2), "update_rule"),
                                     (dict(occupied_threshold=1.0), "occupied_threshold")])
def test_create_refuses_bad_parameters_before_any_device_work(kw, word):
    L = capi.lib()
    out = C.c_void_p(1)
    p = _params(**kw)
    assert L.mh_occmap_create(None, C.byref(p), C.byref(out)) == 1  # MH_ERR_INVALID_ARGUMENT (no context was ever touched)
    assert word in L.mh_last_error_string().decode() and not out.value


def test_null_arguments_are_refused():
    L = capi.lib()
    out, good = C.c_void_p(), _params()
    T = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    assert L.mh_occmap_create(None, C.byref(good), C.byref(out)) == 1 and "null argument" in L.mh_last_error_string().decode()
    assert L.mh_occmap_create(None, None, C.byref(out)) == 1
    assert L.mh_occmap_create(None, C.byref(good), None) == 1
    assert L.mh_occmap_insert(None, None, T, 0.0) == 1
    assert L.mh_occmap_clear(None) == 1
    assert L.mh_occmap_get_info(None, C.byref(capi.OccMapInfo())) == 1
    assert L.mh_occmap_download(None, None, None) == 1
    assert L.mh_occmap_search_map(None, 1.0, C.byref(out)) == 1
    assert L.mh_occmap_destroy(None) == 0  # (like the other destroyers)


# ------------------------------------------------------------------------------------------------ driver
@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def test_inline_lidar2d_pipeline_initialises(host):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(lidar2d_inline.pipeline()))
    d = lo.describePipeline()
    assert d["plan"] == "general" and d["map:localmap"] == "mrpt::maps::CVoxelMap" and d["merge:decimated"] == "localmap"
    assert d["icp_path"] == "layers"  # one point pair with pairingsPerPoint 2: the fused k-best route
    assert lo.localMapSizes() == {"localmap": 0}
    v = lo.downloadVoxelMap("localmap")  # not created before the first key-frame: empty
    assert v["keys"].shape == (0, 3) and len(v["logodds"]) == 0


def test_the_reference_lidar2d_file_initialises(host):
    if not os.path.exists(REF_LIDAR2D):
        pytest.skip("reference tree not present on this box")
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(REF_LIDAR2D))
    d = lo.describePipeline()
    assert d["plan"] == "general" and d["map_class"] == "mrpt::maps::CVoxelMap" and d["icp_path"] == "layers"


def test_an_unknown_map_class_is_still_refused(host):
    text = lidar2d_inline.pipeline(lidar2d_inline.VOXELMAP.format(resolution=0.05).replace("mrpt::maps::CVoxelMap", "mrpt::maps::COctoMap"))
    with pytest.raises(RuntimeError, match="local map class 'mrpt::maps::COctoMap'.*CVoxelMap"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(text))


def test_voxelmap_update_switch_parses(host, monkeypatch):
    monkeypatch.delenv("MOLA_HIP_VOXELMAP_UPDATE", raising=False)
    try:
        host.reload_plugin_switches()
        assert host.plugin_switch_voxelmap_update() == capi.OCC_COUNTED
        for text, want in (("once", capi.OCC_ONCE), ("counted", capi.OCC_COUNTED), ("1", capi.OCC_ONCE)):
            monkeypatch.setenv("MOLA_HIP_VOXELMAP_UPDATE", text)
            host.reload_plugin_switches()
            assert host.plugin_switch_voxelmap_update() == want
    finally:
        monkeypatch.delenv("MOLA_HIP_VOXELMAP_UPDATE", raising=False)
        host.reload_plugin_switches()
