"""Erasing moving objects from the live local map, the parts that need no device: the third public header and its binding, the
online_map_cleaning: options, the ring and neighbour rule of mola_hip::LiveRing against its fold in tests/live_ref.py -- exactly
--, the driver's refusals, and the restatement alone on the two scenarios of tests/live_cases.py -- a condition on the scenarios,
checked before the device is held to them (tests/test_gpu_live.py, tests/test_gpu_odometry_live.py): with the default options the
cleaned fold's final map holds at most 5 % of the mover points the plain fold's final map holds, and the cleaned fold has erased
at most 1 % of the other points it took in.

Measured here.  The street of clean_cases (20 sweeps, exact poses): plain 1 654 mover points left, cleaned 13 (0.79 %); 518 of
107 576 other points erased (0.48 %).  The drive of live_cases (40 sweeps de-skewed with the exact twists, exact poses): plain 817,
cleaned 3 (0.37 %); 315 of 32 443 others erased (0.97 %).  profiles/online_map_cleaning.md says how the drive was settled."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clean_cases as cc
import clean_ref as cr
import live_cases as lc
import live_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_live.h")
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def lv():
    from mola_lidar_odometry_amd import capi_live
    return capi_live


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_third_header_is_declared_exported_and_bound(lv):
    from mola_lidar_odometry_amd import capi, capi_clean
    fns = declared()
    assert fns == sorted(lv._SIGNATURES) and len(fns) == 6
    assert not set(fns) & set(capi._SIGNATURES) and not set(fns) & set(capi_clean._SIGNATURES)   # a table of its own
    L = lv.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_live_api_version()) == lv.LIVE_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7 and int(L.mh_clean_api_version()) == 1   # the other two versions are untouched
    assert len(capi._SIGNATURES) == 82 and len(capi_clean._SIGNATURES) == 7
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):       # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d


def test_the_header_compiles_as_c(lv, tmp_path):
    prog = tmp_path / "live.c"
    prog.write_text(r'''
#include <stdio.h>
#include "molahip_live.h"
int main(void){ printf("%d %d %d\n", MH_LIVE_API_VERSION, MH_LIVE_MAX_VIEWS, MH_CLEAN_API_VERSION); return 0; }''')
    exe = tmp_path / "live"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [1, lv.MAX_VIEWS, 1] and lv.MAX_VIEWS == 64


def test_null_arguments_are_refused_without_a_device(lv):
    L = lv.lib()
    n = C.c_uint64(0)
    assert L.mh_views_put_scan(None, 0, None) == 1
    assert L.mh_views_vote_map(None, None, 0, None, None, None, 0, 0) == 1
    assert L.mh_map_erase_points(None, None, 0, 0) == 1
    assert L.mh_map_erase_seen_through(None, None, 0, None, None, 2, 1) == 1
    assert L.mh_map_erased_total(None, C.byref(n)) == 1


# ---- options -----------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(enabled=False, n_rings=32, n_sectors=128, el_min_deg=-25.0, el_max_deg=15.0, min_range=2.0, max_range=60.0, rel_margin=0.10,
                origin_x=0.0, origin_y=0.0, origin_z=0.0, win_rings=0, win_sectors=1, max_view_distance=30.0, max_views=24,
                min_through_votes=2, agree_weight=1, every_n_updates=1, view_layer="", target_maps=[])


def _opts(host, text):
    d = host.online_map_cleaning_options(text)
    d.pop("device_params")
    return d


def test_the_defaults_are_the_documented_ones_and_map_cleaning_s(host):
    assert _opts(host, None) == DEFAULTS == _opts(host, "online_map_cleaning:\n") == _opts(host, host.Config.FromYamlText("other: 1\n"))
    shared = [k for k in DEFAULTS if k not in ("enabled", "max_views", "every_n_updates", "view_layer", "target_maps")]
    off_line = host.map_cleaning_options(None)
    assert {k: DEFAULTS[k] for k in shared} == {k: off_line[k] for k in shared}
    assert host.online_map_cleaning_options(None)["device_params"] == off_line["device_params"]
    assert lr.HOST_DEFAULT == {k: DEFAULTS[k] for k in lr.HOST_DEFAULT}


def test_every_key_is_read(host):
    text = ("online_map_cleaning:\n  enabled: true\n  n_rings: 16\n  n_sectors: 64\n  el_min_deg: -30\n  el_max_deg: 10.5\n  min_range: 1.5\n"
            "  max_range: 80\n  rel_margin: 0.2\n  origin_x: 0.1\n  origin_y: -0.2\n  origin_z: 1.7\n  win_rings: 1\n  win_sectors: 2\n"
            "  max_view_distance: 12.5\n  max_views: 8\n  min_through_votes: 3\n  agree_weight: 2\n  every_n_updates: 4\n"
            "  view_layer: decimated_for_icp\n  target_maps: [localmap, other]\n")
    assert _opts(host, text) == dict(enabled=True, n_rings=16, n_sectors=64, el_min_deg=-30.0, el_max_deg=10.5, min_range=1.5, max_range=80.0,
                                     rel_margin=0.2, origin_x=0.1, origin_y=-0.2, origin_z=1.7, win_rings=1, win_sectors=2,
                                     max_view_distance=12.5, max_views=8, min_through_votes=3, agree_weight=2, every_n_updates=4,
                                     view_layer="decimated_for_icp", target_maps=["localmap", "other"])
    dev = host.online_map_cleaning_options(text)["device_params"]
    assert dev[:2] == (16, 64) and dev[2] == float(np.float32(np.radians(-30.0))) and dev[7] == tuple(float(np.float32(v)) for v in (0.1, -0.2, 1.7))


@pytest.mark.parametrize("line,message", [
    ("n_rings: 0", "online_map_cleaning: n_rings must be in 1..64"), ("n_rings: 65", "online_map_cleaning: n_rings must be in 1..64"),
    ("n_sectors: 12", "online_map_cleaning: n_sectors must be a multiple of 8 in 8..256"),
    ("n_rings: 64\n  n_sectors: 128", "online_map_cleaning: n_sectors times n_rings must be <= 4096"),
    ("el_min_deg: -90", "online_map_cleaning: el_min_deg must lie inside (-90, 90)"),
    ("el_max_deg: -30", "online_map_cleaning: el_max_deg must lie inside (el_min_deg, 90)"),
    ("min_range: 0", "online_map_cleaning: min_range must be finite and > 0"),
    ("max_range: 1", "online_map_cleaning: max_range must be finite and > min_range"),
    ("rel_margin: 0", "online_map_cleaning: rel_margin must be finite and > 0"),
    ("origin_y: inf", "online_map_cleaning: origin_y must be finite"),
    ("win_rings: 3", "online_map_cleaning: win_rings must be in 0..2"), ("win_sectors: 3", "online_map_cleaning: win_sectors must be in 0..2"),
    ("max_view_distance: -1", "online_map_cleaning: max_view_distance must be finite and >= 0"),
    ("min_through_votes: 0", "online_map_cleaning: min_through_votes must be an integer >= 1"),
    ("agree_weight: -1", "online_map_cleaning: agree_weight must be an integer >= 0"),
    ("agree_weight: 1.5", "online_map_cleaning: agree_weight must be an integer >= 0"),
    ("max_views: 0", "online_map_cleaning: max_views must be in 1..64"), ("max_views: 65", "online_map_cleaning: max_views must be in 1..64"),
    ("every_n_updates: 0", "online_map_cleaning: every_n_updates must be an integer >= 1"),
    ("enabled: perhaps", "online_map_cleaning: enabled must be true or false"),
    ("n_rings: many", "online_map_cleaning: n_rings must be a number"),
    ("max_views_per_frame: 3", "online_map_cleaning: max_views_per_frame is not a key of this block"),
    ("target_maps: localmap", "online_map_cleaning: target_maps must be a list of map names"),
    ("target_maps: [a, a]", "online_map_cleaning: target_maps names 'a' twice"),
])
def test_every_refusal_names_the_block_and_the_key(host, line, message):
    with pytest.raises(RuntimeError) as e:
        host.online_map_cleaning_options("online_map_cleaning:\n  %s\n" % line)
    assert str(e.value) == message
    with pytest.raises(RuntimeError) as e:   # the driver reads and checks the block whether it is enabled or not
        host.LidarOdometry().initialize(host.Config.FromYamlText(open(PIPE).read() + "\nonline_map_cleaning:\n  %s\n" % line))
    assert str(e.value) == message


def _init(host, block, text=None, edit=lambda t: t):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(edit(open(PIPE).read() if text is None else text) + block))
    return lo


def test_the_driver_refuses_by_name_what_it_cannot_clean(host):
    on = "\nonline_map_cleaning:\n  enabled: true\n"
    assert _init(host, on).onlineMapCleaningOptions()["enabled"] and not _init(host, "").onlineMapCleaningOptions()["enabled"]
    assert _init(host, on + "  target_maps: [localmap]\n  view_layer: decimated_for_map\n").mapPointsErased() == 0
    with pytest.raises(RuntimeError, match="online_map_cleaning: target_maps names 'nomap', which is no local map of this pipeline"):
        _init(host, on + "  target_maps: [nomap]\n")
    with pytest.raises(RuntimeError, match="online_map_cleaning: view_layer 'nolayer' is no observation layer this pipeline's filters make"):
        _init(host, on + "  view_layer: nolayer\n")
    gen = lambda t: t.replace("generate: ${MOLA_GENERATE_SIMPLEMAP|false}", "generate: true").replace("${MOLA_SIMPLEMAP_OUTPUT|'final_map.simplemap'}", "''")
    with pytest.raises(RuntimeError, match="online_map_cleaning: enabled together with online_loop_closure: correct_driver: true is not implemented"):
        _init(host, on + "\nonline_loop_closure:\n  enabled: true\n", edit=gen)
    _init(host, on + "\nonline_loop_closure:\n  enabled: true\n  correct_driver: false\n", edit=gen)   # a closer that only reports is fine
    _init(host, "\nonline_map_cleaning:\n  enabled: false\n\nonline_loop_closure:\n  enabled: true\n", edit=gen)
    import lidar2d_inline   # an occupancy map stores no points to erase
    with pytest.raises(RuntimeError, match="online_map_cleaning: enabled, but every local map of this pipeline is a 'CVoxelMap'"):
        _init(host, on, text=lidar2d_inline.pipeline())
    with pytest.raises(RuntimeError, match="online_map_cleaning: target map 'localmap' is a 'CVoxelMap'"):
        _init(host, on + "  target_maps: [localmap]\n", text=lidar2d_inline.pipeline())
    lo = _init(host, on)
    with pytest.raises(RuntimeError, match="setAlignBatcher: not available with online_map_cleaning: enabled is not available with an AlignBatcher"):
        lo.setAlignBatcher(host.AlignBatcher(2))


# ---- the ring and the neighbour rule -------------------------------------------------------------------------------------------------
def _fold(poses, **host_opts):
    """the rule's host half in Python: per update (slot, due, neighbour slots)"""
    h = dict(lr.HOST_DEFAULT, **host_opts)
    ring, out = {}, []
    for u, T in enumerate(poses):
        slot = u % h["max_views"]
        ring[slot] = (None, T)
        due = (u + 1) % h["every_n_updates"] == 0
        out.append((slot, due, lr.ring_neighbours(ring, T, **h) if due else []))
    return out


def _block(**o):
    return "online_map_cleaning:\n" + "".join("  %s: %r\n" % kv for kv in o.items())


def _pose(x, y=0.0, z=0.0):
    return np.array([1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z], np.float64)


def test_the_ring_rule_on_hand_made_pose_lists(host):
    line = np.array([_pose(3.0 * k) for k in range(10)])
    got = host.live_ring_fold(line, _block(max_views=4, max_view_distance=6.0))
    assert [tuple(g) for g in got] == [(s, d, list(n)) for s, d, n in _fold(line, max_views=4, max_view_distance=6.0)]
    assert [g[0] for g in got] == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]                      # the ring wraps at max_views
    assert list(got[2][2]) == [0, 1, 2] and list(got[3][2]) == [1, 2, 3]              # 6 m: closed (the slot 6 m back is in)
    assert list(got[5][2]) == [0, 1, 3]                                               # after the wrap: slots 3, 0, 1 hold updates 3, 4, 5
    assert list(got[9][2]) == [0, 1, 3]
    every = host.live_ring_fold(line, _block(max_views=4, max_view_distance=100.0, every_n_updates=3))
    assert [g[1] for g in every] == [False, False, True] * 3 + [False] and all(not list(g[2]) for g in every if not g[1])
    assert list(every[2][2]) == [0, 1, 2] and list(every[8][2]) == [0, 1, 2, 3]
    assert [tuple(g) for g in every] == [(s, d, list(n)) for s, d, n in _fold(line, max_views=4, max_view_distance=100.0, every_n_updates=3)]
    # a revisit: the start comes back within reach; vertical distance counts
    loop = np.array([_pose(0, 0), _pose(20, 0), _pose(20, 20), _pose(0, 20), _pose(0, 1), _pose(0, 1, 29.9), _pose(0, 1, 31.1)])
    got = host.live_ring_fold(loop, _block(max_views=24))
    assert [list(g[2]) for g in got] == [n for _, _, n in _fold(loop)]
    assert list(got[4][2]) == [0, 1, 2, 3, 4] and list(got[5][2]) == [0, 4, 5] and list(got[6][2]) == [5, 6]
    assert list(host.live_ring_fold(line[:3], _block(max_view_distance=0.0))[2][2]) == [2]   # the update's own slot is always in


def test_the_ring_rule_on_200_random_pose_lists(host):
    rng = np.random.default_rng(77)
    for _ in range(200):
        n, mv, every = int(rng.integers(1, 40)), int(rng.integers(1, 12)), int(rng.integers(1, 5))
        dist = float(rng.choice([0.0, 5.0, 10.0, 30.0]))
        steps = rng.normal(0, 3.0, (n, 3)).round(int(rng.integers(0, 3)))   # (rounded steps: distances exactly on the limit occur)
        poses = np.array([_pose(*p) for p in np.cumsum(steps, 0)])
        got = host.live_ring_fold(poses, _block(max_views=mv, every_n_updates=every, max_view_distance=dist))
        assert [(g[0], g[1], list(g[2])) for g in got] == _fold(poses, max_views=mv, every_n_updates=every, max_view_distance=dist)


# ---- a condition on the scenarios, on the restatement alone ----------------------------------------------------------------------------
def _condition(sweeps, poses, mover):
    plain, _ = lc.fold(sweeps, poses, mover, clean=False)
    cleaned, f = lc.fold(sweeps, poses, mover)
    left, _, erased_others, others = cleaned
    print("plain: %d mover points left; cleaned: %d left (%.2f %%), %d of %d others erased (%.2f %%), %d erased in all"
          % (plain[0], left, 100.0 * left / plain[0], erased_others, others, 100.0 * erased_others / others, f.erased))
    assert plain[0] > 500                                  # (there is a trail to lose)
    assert left <= 0.05 * plain[0]
    assert erased_others <= 0.01 * others
    return plain, cleaned


def test_the_restatement_cleans_the_street_of_clean_cases():
    """measured: plain 1 654 mover points left, cleaned 13 (0.79 %); 518 of 107 576 others erased (0.48 %)"""
    s = cc.scenario()
    assert lc.MAP_ARGS[:2] == (cc.MAP_PARAMS["voxel_size"], cc.MAP_PARAMS["max_points_per_voxel"])
    _condition(s["sweeps"], s["poses"], s["mover"])


def test_the_restatement_cleans_the_drive_with_exact_poses():
    """measured: plain 817 mover points left, cleaned 3 (0.37 %); 315 of 32 443 others erased (0.97 %)"""
    _condition(*lc.drive_deskewed())
