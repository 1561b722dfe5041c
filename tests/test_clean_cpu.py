"""Map cleaning, the parts that need no device: the second public header and its binding, the map_cleaning: options, the host
rules (mola_hip::cleaning_neighbours, the relative pose, the decision) against their folds in tests/clean_ref.py -- exactly --,
the restatement's own binding properties, the refusals, and the restatement alone on the scenario of tests/clean_cases.py -- a
condition on the scenario: with the default options it must lose at least 90 % of the mover's points and at most 1 % of the
others before the device is held to it (tests/test_gpu_clean.py).

Measured here: 9 790 mover points of which 9 763 go (99.7 %); 356 452 other points of which 361 go (0.10 %); profiles/map_cleaning.md
says how the scenario and the default window were settled."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clean_cases as cc
import clean_ref as cr
import loop_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_clean.h")
I12 = np.eye(4)[:3].reshape(12)


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def cl():
    from mola_lidar_odometry_amd import capi_clean
    return capi_clean


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_second_header_is_declared_exported_and_bound(cl):
    from mola_lidar_odometry_amd import capi
    fns = declared()
    assert fns == sorted(cl._SIGNATURES) and len(fns) == 7
    assert not set(fns) & set(capi._SIGNATURES)                      # nothing of it went into the first header's table
    L = cl.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_clean_api_version()) == cl.CLEAN_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                              # the first header's version is untouched
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):       # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(cl, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_clean.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_clean_params), offsetof(mh_clean_params, n_rings),
    offsetof(mh_clean_params, n_sectors), offsetof(mh_clean_params, el_min), offsetof(mh_clean_params, el_max),
    offsetof(mh_clean_params, min_range), offsetof(mh_clean_params, max_range), offsetof(mh_clean_params, rel_margin),
    offsetof(mh_clean_params, origin), offsetof(mh_clean_params, win_rings), offsetof(mh_clean_params, win_sectors));
  printf("%d %d %d %d %u %zu\n", MH_CLEAN_API_VERSION, MH_CLEAN_MAX_RINGS, MH_CLEAN_MAX_SECTORS, MH_CLEAN_MAX_BINS, MH_CLEAN_EMPTY, sizeof(mh_map_frame));
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    P = cl.CleanParams
    assert [int(v) for v in a.split()] == [C.sizeof(P), P.n_rings.offset, P.n_sectors.offset, P.el_min.offset, P.el_max.offset, P.min_range.offset,
                                           P.max_range.offset, P.rel_margin.offset, P.origin.offset, P.win_rings.offset, P.win_sectors.offset]
    assert C.sizeof(P) == 48
    assert [int(v) for v in b.split()] == [1, 64, 256, 4096, cl.EMPTY, 128]


def test_calls_fail_loudly_without_a_device(cl):
    from mola_lidar_odometry_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(capi.MolahipError) as e:
        cl.Views(capi.Context(0), cl.clean_params())
    assert e.value.status == 5
    h = C.c_void_p()
    assert cl.lib().mh_views_create(None, C.byref(cl.clean_params()), C.byref(h)) == 1    # refusals need no device


# ---- options -----------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(n_rings=32, n_sectors=128, el_min_deg=-25.0, el_max_deg=15.0, min_range=2.0, max_range=60.0, rel_margin=0.10, origin_x=0.0,
                origin_y=0.0, origin_z=0.0, win_rings=0, win_sectors=1, max_view_distance=30.0, max_views_per_frame=24, min_through_votes=2,
                agree_weight=1)


def _opts(host, text):
    d = host.map_cleaning_options(text)
    d.pop("device_params")
    return d


def test_the_defaults_are_the_documented_ones_and_the_restatement_s(host):
    assert _opts(host, None) == DEFAULTS == _opts(host, "map_cleaning:\n") == _opts(host, host.Config.FromYamlText("other: 1\n"))
    dev = host.map_cleaning_options(None)["device_params"]
    R = cr.DEFAULT
    F = np.float32
    assert dev == (R["n_rings"], R["n_sectors"], float(F(R["el_min"])), float(F(R["el_max"])), R["min_range"], R["max_range"],
                   float(F(R["rel_margin"])), R["origin"], R["win_rings"], R["win_sectors"])
    assert {k: DEFAULTS[k] for k in cr.HOST_DEFAULT} == cr.HOST_DEFAULT


@pytest.mark.parametrize("key,value", [("n_rings", 16), ("n_sectors", 64), ("el_min_deg", -30.5), ("el_max_deg", 2.5), ("min_range", 1.5),
                                       ("max_range", 80.0), ("rel_margin", 0.2), ("origin_x", 0.5), ("origin_y", -0.25), ("origin_z", 1.75),
                                       ("win_rings", 2), ("win_sectors", 2), ("max_view_distance", 12.5), ("max_views_per_frame", 8),
                                       ("min_through_votes", 3), ("agree_weight", 0)])
def test_each_key_is_read(host, key, value):
    assert _opts(host, "map_cleaning:\n  %s: %s\n" % (key, value)) == dict(DEFAULTS, **{key: value})


@pytest.mark.parametrize("key,value", [("n_rings", 0), ("n_rings", 65), ("n_rings", 1.5), ("n_sectors", 12), ("n_sectors", 264), ("n_sectors", 256),
                                       ("el_min_deg", -90), ("el_min_deg", 95), ("el_max_deg", 90), ("el_max_deg", -30), ("min_range", 0),
                                       ("min_range", "nan"), ("max_range", 1.0), ("max_range", "inf"), ("rel_margin", 0), ("rel_margin", -0.1),
                                       ("origin_y", "nan"), ("win_rings", 3), ("win_sectors", -1), ("max_view_distance", -1),
                                       ("max_view_distance", "abc"), ("max_views_per_frame", 0), ("min_through_votes", 0), ("agree_weight", -1),
                                       ("agree_weight", 0.5), ("no_such_key", 1), ("max_views", 4)])
def test_a_bad_value_or_an_unknown_key_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"map_cleaning: %s\b" % key):
        host.map_cleaning_options("map_cleaning:\n  %s: %s\n" % (key, value))


# ---- the neighbour rule, the relative pose, the decision ---------------------------------------------------------------------------
def _line(xs):
    return np.array([[1, 0, 0, x, 0, 1, 0, 0.0, 0, 0, 1, 0.0] for x in xs], np.float64)


def _same_neighbours(host, poses, has, **opt):
    text = "map_cleaning:\n" + "".join("  %s: %s\n" % kv for kv in opt.items()) if opt else None
    got = host.cleaning_neighbours(poses, list(has), text)
    want = cr.neighbours(poses, has, **dict(cr.HOST_DEFAULT, **opt))
    assert [list(g) for g in got] == want
    return want


def test_the_neighbour_rule_on_hand_made_cases(host):
    # ties at equal distance go to the lower index; the list comes back in index order
    assert _same_neighbours(host, _line([0, -3, 3, -6, 6]), [True] * 5, max_views_per_frame=3) == [[1, 2, 3], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 1, 2]]
    # the cap keeps the nearest; the distance is closed
    assert _same_neighbours(host, _line([0, 10, 20, 30, 30.5]), [True] * 5, max_views_per_frame=2)[0] == [1, 2]
    assert _same_neighbours(host, _line([0, 10, 20, 30, 30.5]), [True] * 5)[0] == [1, 2, 3]
    # frames without points neither vote nor are voted against
    assert _same_neighbours(host, _line([0, 1, 2, 3]), [True, False, True, True]) == [[2, 3], [], [0, 3], [0, 2]]
    # a single frame, no frame, coinciding frames
    assert _same_neighbours(host, _line([5]), [True]) == [[]]
    assert _same_neighbours(host, np.zeros((0, 12)), []) == []
    assert _same_neighbours(host, _line([1, 1, 1]), [True] * 3, max_views_per_frame=1) == [[1], [0], [0]]
    assert _same_neighbours(host, _line([0, 40]), [True] * 2) == [[], []]


def test_the_neighbour_rule_on_random_pose_sets(host):
    rng = np.random.default_rng(77)
    for trial in range(200):
        K = int(rng.integers(1, 40))
        poses = np.array([cr_pose(rng) for _ in range(K)])
        if trial % 3 == 0:  # a lattice: many equal distances
            poses[:, [3, 7, 11]] = rng.integers(-3, 4, (K, 3)) * 4.0
        has = rng.uniform(size=K) < 0.85
        _same_neighbours(host, poses, has, max_view_distance=float(rng.choice([0.0, 8.0, 12.0, 30.0])), max_views_per_frame=int(rng.integers(1, 9)))


def cr_pose(rng):
    from mola_lidar_odometry_amd import synth
    return np.asarray(synth.pose_from_ypr(np.concatenate([rng.uniform(-15, 15, 3), rng.uniform(-np.pi, np.pi, 3)]))).reshape(12)


def test_the_relative_pose_is_the_header_s_formula(host):
    rng = np.random.default_rng(3)
    for _ in range(50):
        Ti, Tj = cr_pose(rng), cr_pose(rng)
        got = np.array(host.cleaning_relative_pose(list(Ti), list(Tj)))
        assert got.tobytes() == cr.relative_pose(Ti, Tj).tobytes()
        assert np.abs(got - lc.relative(Tj, Ti)).max() < 1e-12
    assert np.array(host.cleaning_relative_pose(list(I12), list(I12))).tobytes() == I12.tobytes()


def test_the_decision_is_integer_arithmetic(host):
    th, ag = np.meshgrid(np.array([0, 1, 2, 3, 5, 65535], np.uint32), np.array([0, 1, 2, 3, 4, 65535], np.uint32))
    votes = (th | ag << 16).reshape(-1)
    for text, kw in ((None, {}), ("map_cleaning:\n  min_through_votes: 1\n  agree_weight: 0\n", dict(min_through_votes=1, agree_weight=0)),
                     ("map_cleaning:\n  min_through_votes: 3\n  agree_weight: 2\n", dict(min_through_votes=3, agree_weight=2))):
        assert list(host.cleaning_removes(votes, text)) == list(cr.decide(votes, **dict(cr.HOST_DEFAULT, **kw)))
    assert list(host.cleaning_removes(np.array([2, 2 | 2 << 16, 3 | 2 << 16, 1], np.uint32), None)) == [True, False, True, False]


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------
def test_a_view_does_not_depend_on_the_order_of_its_points():
    p = dict(cr.DEFAULT)
    c = cr.edge_cloud(6000, 1, **p)
    v = cr.view(c, **p)
    assert (v != cr.EMPTY).sum() > 1000
    for seed in range(3):
        assert (cr.view(c[np.random.default_rng(seed).permutation(len(c))], **p) == v).all()


@pytest.mark.parametrize("S", [8, 64, 128])
def test_a_quarter_turn_shifts_the_restatement_s_view_by_a_quarter_of_its_columns(S):
    p = dict(cr.DEFAULT, n_sectors=S)
    c = cr.edge_cloud(6000, 2, **p)
    v, t = cr.view(c, **p), c
    for q in range(1, 5):
        t = cr.quarter_turn(t)
        assert (cr.view(t, **p) == np.roll(v, q * S // 4, axis=1)).all(), (S, q)


def test_a_frame_collects_no_through_vote_against_its_own_view():
    for kw in (dict(), dict(win_rings=0, win_sectors=0), dict(win_rings=2, win_sectors=2, n_rings=8, n_sectors=64), dict(rel_margin=1e-4)):
        p = dict(cr.DEFAULT, **kw)
        c = cr.edge_cloud(6000, 4, **p)
        v = cr.vote(c, [cr.view(c, **p)], [0], [I12], **p)
        assert not (v & 0xFFFF).any() and (v >> 16).sum() > 300


def test_the_counters_of_the_restatement_saturate():
    p = dict(cr.DEFAULT, win_rings=0, win_sectors=0)
    q = np.array([[4, 0, 0], [0, 10, 0]], np.float32)
    img = cr.view(np.array([[9, 0, 0], [0, 10.2, 0]], np.float32), **p)
    assert list(cr.vote(q, [img], [0, 0], [I12, I12], weights=[65534, 1], **p)) == [65535, 65535 << 16]
    assert list(cr.vote(q, [img], [0], [I12], weights=[70000], **p)) == [65535, 65535 << 16]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _tiny(n, points=True):
    rng = np.random.default_rng(0)
    kf = cc.keyframe_set(_line(2.0 * np.arange(n)), [rng.uniform(-20, 20, (50, 3)).astype(np.float32) for _ in range(n)])
    if not points:
        for f in kf["frames"]:
            f["layers"] = None
    return kf


def test_a_header_with_an_occupancy_map_is_refused_and_a_good_one_asks_for_the_device(host):
    from mola_lidar_odometry_amd import capi
    kf = _tiny(3)
    kf["maps"][0]["class_name"] = "CVoxelMap"
    with pytest.raises(RuntimeError, match=r"clean_keyframes: target map 'localmap' is a 'CVoxelMap': an occupancy map"):
        host.clean_keyframes(kf, None)
    with pytest.raises(RuntimeError, match=r"map_cleaning: win_rings\b"):
        host.clean_keyframes(_tiny(3), "map_cleaning:\n  win_rings: 5\n")
    if capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            host.clean_keyframes(_tiny(3), None)


def test_a_set_without_points_comes_back_unchanged_without_a_device(host, tmp_path):
    kf = _tiny(4, points=False)
    back, report = host.clean_keyframes(kf, None)
    a, b = str(tmp_path / "a.mhkf"), str(tmp_path / "b.mhkf")
    host.write_keyframe_file(a, kf)
    host.write_keyframe_file(b, back)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert report["points_in"] == 0 and report["points_removed"] == 0 and report["pairs"] == 0 and len(report["frames"]) == 4
    back, report = host.clean_keyframes(dict(maps=kf["maps"], frames=[]), None)
    assert back["frames"] == [] and report["frames"] == []


# ---- the scenario, by the restatement alone ----------------------------------------------------------------------------------------
def test_the_scenario_meets_its_two_conditions_with_the_default_options():
    sc = cc.scenario()
    assert len(sc["sweeps"]) == 20 and all(m.any() for m in sc["mover"])
    masks, votes, nb = cr.clean(sc["sweeps"], sc["poses"])
    mv, rm = np.concatenate(sc["mover"]), np.concatenate(masks)
    print("mover points", int(mv.sum()), "removed", int((mv & rm).sum()), "| other points", int((~mv).sum()), "removed", int((~mv & rm).sum()))
    print("neighbours per frame", [len(n) for n in nb])
    assert (mv & rm).sum() >= 0.90 * mv.sum()
    assert (~mv & rm).sum() <= 0.01 * (~mv).sum()
