"""Place recognition, the checks that need no GPU: the seven entry points are declared, exported and bound and the ABI number
stays; tests/place_ref.py -- the numpy restatement the device is held to -- has the properties the header promises; the new
options parse with their defaults; relocalizeInKeyFrames refuses what relocalizeNearPose refuses; and the reference alone
(tests/place_localize_ref.py on the CPU oracle) finds the three places of tests/test_odometry_place.py within its bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import place_cases as pc
import place_ref as pr
from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")
PIPES = [os.path.join(ROOT, "pipelines", n) for n in ("lidar3d-default-hip.yaml", "lidar3d-ndt-hip.yaml")]
NEW = ["mh_place_describe", "mh_place_db_create", "mh_place_db_destroy", "mh_place_db_size", "mh_place_db_add", "mh_place_db_add_frames",
       "mh_place_search"]
F = np.float32


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def test_the_seven_symbols_are_declared_exported_and_bound():
    declared = set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read()))
    L = capi.lib()
    for fn in NEW:
        assert fn in declared and hasattr(L, fn) and fn in capi._SIGNATURES, fn
    assert int(L.mh_abi_version()) == 7
    assert (capi.PLACE_MAX_RINGS, capi.PLACE_MAX_SECTORS, capi.PLACE_MAX_DESCRIPTORS) == (32, 128, 1048576)


def test_every_entry_point_from_before_stays_exported():
    """the declared set of the parent commit, by name (74 entry points + the seven new ones = 81; `later`: added since, by name)"""
    L = capi.lib()
    later = ["mh_debug_flat_stats"]
    assert all(n in capi._SIGNATURES for n in later)
    before = [n for n in capi._SIGNATURES if n not in NEW and n not in later]
    assert len(before) == 74 and len(capi._SIGNATURES) == 81 + len(later)
    for must in ("mh_score_poses", "mh_map_insert_frames", "mh_map_restore", "mh_nn_search_radius", "mh_icp_align", "mh_scan_create"):
        assert must in before
    assert all(hasattr(L, n) for n in before)


def test_struct_sizes_from_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "molahip.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", '
                    'sizeof(mh_place_params), sizeof(mh_place_match), offsetof(mh_place_params, min_range), offsetof(mh_place_match, dist)); '
                    'return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [24, 8, 8, 4]
    assert got == [C.sizeof(capi.PlaceParams), C.sizeof(capi.PlaceMatch), capi.PlaceParams.min_range.offset, capi.PlaceMatch.dist.offset]
    assert capi.PLACE_MATCH_DTYPE.itemsize == 8


# ---- the restatement itself
def _cloud(n, seed, z=(-2.0, 20.0)):
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(-np.pi, np.pi, n), rng.uniform(1.5, 79.0, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(z[0], z[1], n)], 1).astype(F)


@pytest.mark.parametrize("R,S", [(20, 64), (1, 8), (32, 128), (5, 24)])
def test_ref_quarter_turn_shifts_by_a_quarter(R, S):
    p = dict(pr.DEFAULT, n_rings=R, n_sectors=S)
    xyz = pr.edge_cloud(5000, 3, **p)
    d = pr.describe(xyz, **p)
    t = xyz
    for q in range(1, 5):
        t = pr.quarter_turn(t)
        assert np.array_equal(pr.describe(t, **p), np.roll(d, q * S // 4, axis=1)), q
    assert d.any()


@pytest.mark.parametrize("S", [8, 64, 128])
def test_ref_sectors_agree_with_arctan2_away_from_the_boundaries(S):
    p = dict(pr.DEFAULT, n_sectors=S)
    xyz = _cloud(20000, 5)
    keep, ring, sector, level = pr.bins(xyz, **p)
    f = np.arctan2(xyz[:, 1].astype(np.float64), xyz[:, 0].astype(np.float64)) * S / (2 * np.pi)
    away = np.abs(f - np.round(f)) > 1e-4
    assert keep.all() and away.sum() > 19000
    assert np.array_equal(sector[away], np.floor(f[away]).astype(np.int64) % S)
    assert set(sector.tolist()) == set(range(S))   # every sector is hit
    rr = np.sqrt((xyz[:, 0].astype(np.float64)) ** 2 + xyz[:, 1].astype(np.float64) ** 2)
    fr = (rr - 1.0) / 79.0 * 20
    inside = np.abs(fr - np.round(fr)) > 1e-4
    assert np.array_equal(ring[inside], np.floor(fr[inside]).astype(np.int64))
    lv = 1 + np.floor((xyz[:, 2].astype(np.float64) + 3.0) * 254.0 / 30.0)
    assert np.abs(level - lv).max() <= 1 and (level == lv).mean() > 0.99


def test_ref_axes_and_diagonals_lie_on_the_closed_lower_end():
    S = 64
    p = dict(pr.DEFAULT, n_sectors=S)
    a = F(10.0)
    pts = np.array([(a, 0, 0), (a, a, 0), (0, a, 0), (-a, a, 0), (-a, 0, 0), (-a, -a, 0), (0, -a, 0), (a, -a, 0)], F)
    keep, _, sector, _ = pr.bins(pts, **p)
    assert keep.all() and sector.tolist() == [k * S // 8 for k in range(8)]
    eps = np.array([(a, -1e-4, 0), (a, np.nextafter(a, F(0)), 0), (1e-4, a, 0)], F)   # just below: the sector before
    assert pr.bins(eps, **p)[2].tolist() == [S - 1, S // 8 - 1, S // 4 - 1]
    # the skipped points: the origin, non-finite coordinates, outside the annulus, outside [z_min, z_max)
    bad = np.array([(0, 0, 0), (np.nan, 1, 0), (5, np.inf, 0), (5, 5, np.nan), (0.5, 0.5, 0), (80, 0, 0), (5, 5, -3.1), (5, 5, 27.0)], F)
    assert not pr.bins(bad, **p)[0].any()
    ok = np.array([(1, 0, -3.0), (0, -1, np.nextafter(F(27.0), F(0))), (np.nextafter(F(80.0), F(0)), 0, 0)], F)
    keep, ring, _, level = pr.bins(ok, **p)
    assert keep.all() and ring.tolist() == [0, 0, 19] and level.tolist() == [1, 254, 26]


def test_ref_search_finds_a_rolled_copy_and_the_smallest_shift_on_ties():
    rng = np.random.default_rng(9)
    R, S = 20, 64
    stored = rng.integers(0, 256, (5, R, S), dtype=np.uint8)
    stored[3] = stored[1]
    for j, s in ((0, 0), (2, 7), (4, S - 1)):
        shift, dist = pr.search(stored, np.roll(stored[j], s, axis=1))
        assert dist[j] == 0 and shift[j] == s and (dist[[k for k in range(5) if k not in (j,)]] > 0).all()
    shift, dist = pr.search(stored, np.roll(stored[1], 11, axis=1))
    assert shift[1] == shift[3] == 11 and dist[1] == dist[3] == 0
    shift, dist = pr.search(stored, np.full((R, S), 99, np.uint8))   # every shift ties
    assert not shift.any() and np.array_equal(dist, np.abs(stored.astype(np.int64) - 99).sum(axis=(1, 2)))
    assert pr.rank(shift, np.array([5, 3, 5, 3, 9])).tolist() == [1, 3, 0, 2, 4]
    period = np.tile(rng.integers(0, 256, (R, 16), dtype=np.uint8), (1, 4))   # a descriptor with period 16: the first of four minima
    assert pr.search(period[None], np.roll(period, 21, axis=1))[0][0] == 5
    assert pr.distances(stored, stored[0]).max() < 1 << 20


# ---- options and refusals of the host layer
@pytest.mark.parametrize("pipe", PIPES)
def test_option_keys_default_as_listed(host, pipe, monkeypatch):
    for v in ("MOLA_LOAD_MM", "MOLA_LOAD_SM"):
        monkeypatch.delenv(v, raising=False)
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(pipe))
    ro = lo.relocalizationOptions()
    want = dict(place_rings=20, place_sectors=64, place_min_range=1.0, place_max_range=80.0, place_z_min=-3.0, place_z_max=27.0,
                place_top_k=4, place_sigma_xy=1.0, place_sigma_yaw_deg=5.625)
    assert {k: ro[k] for k in want} == want
    assert (ro["step_yaw_deg"], ro["sigmas"], ro["refine_top_k"], ro["max_candidates"]) == (3.0, 3.0, 4, 65536)   # the old keys as before
    txt = pc.pipeline_text(pipe).replace("  place_sectors: 64\n", "  place_sectors: 32\n").replace("  place_z_max: 27.0\n", "  place_z_max: 9.5\n")
    lo2 = host.LidarOdometry()
    lo2.initialize(host.Config.FromYamlText(txt))
    ro = lo2.relocalizationOptions()
    assert (ro["place_top_k"], ro["place_sigma_xy"], ro["place_sectors"], ro["place_z_max"], ro["place_rings"]) == (2, 0.5, 32, 9.5, 20)
    for key, bad in (("place_sectors: 64", "place_sectors: 12"), ("place_rings: 20", "place_rings: 33"), ("place_top_k: 2", "place_top_k: 0"),
                     ("place_max_range: 80.0", "place_max_range: 0.5"), ("place_z_min: -3.0", "place_z_min: 30")):
        txt = pc.pipeline_text(pipe)
        assert txt.count("  %s\n" % key) == 1
        with pytest.raises(RuntimeError, match="relocalization: place_rings"):
            host.LidarOdometry().initialize(host.Config.FromYamlText(txt.replace("  %s\n" % key, "  %s\n" % bad)))
    # a pipeline file from before the keys existed parses as it did: the defaults
    import re
    old = re.sub(r"  # LidarOdometry::relocalizeInKeyFrames.*?place_sigma_yaw_deg: 5.625\n", "", open(pipe).read(), flags=re.S)
    assert "place_" not in old
    lo3 = host.LidarOdometry()
    lo3.initialize(host.Config.FromYamlText(old))
    assert {k: lo3.relocalizationOptions()[k] for k in want} == want


def test_relocalize_in_keyframes_refusals(host, monkeypatch):
    for v in ("MOLA_LOAD_MM", "MOLA_LOAD_SM"):
        monkeypatch.delenv(v, raising=False)
    lo = host.LidarOdometry()
    with pytest.raises(RuntimeError, match="before initialize"):
        lo.relocalizeInKeyFrames()
    lo.initialize(host.Config.FromYamlFile(PIPES[0]))
    assert not lo.relocalizationPending()
    lo.relocalizeInKeyFrames()   # accepted: served by the first scan that reaches registration with a non-empty map
    assert lo.relocalizationPending()
    lo.reset()
    assert not lo.relocalizationPending()
    if capi.device_count() > 0:   # (a batch member takes a device context of its own)
        batched = host.LidarOdometry(device=0, own_context=True)
        batched.initialize(host.Config.FromYamlFile(PIPES[0]))
        batcher = host.AlignBatcher(1)
        batched.setAlignBatcher(batcher)
        with pytest.raises(RuntimeError, match="AlignBatcher"):
            batched.relocalizeInKeyFrames()
        batcher.leave()


# ---- the reference alone on the scenario of the GPU test
def test_the_reference_alone_finds_the_three_places(oracle, monkeypatch):
    import place_localize_ref as plr
    for v in ("MOLA_LOAD_MM", "MOLA_LOAD_SM", "MOLA_GENERATE_SIMPLEMAP"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("MOLA_MAPPING_ENABLED", "false")
    monkeypatch.setenv("MOLA_MINIMUM_ICP_QUALITY", pc.MIN_QUALITY)
    sc = pc.scene()
    frames, rec = plr.cpu_session(PIPES[0], sc)
    assert len(frames) == 12 and all(len(f["layers"][0][1]) > 300 for f in frames)
    text = pc.pipeline_text(PIPES[0])
    for q, (xyz, t) in enumerate(pc.query_sweeps(sc) + [pc.sweep(sc, np.array(pc.FAR_QUERY), 300)]):
        o = plr.PlaceOracle(None, text=text)
        o.preload(rec)
        o.set_keyframes(frames)
        o.relocalize_in_keyframes()
        r = o.on_lidar(2000.0, xyz, t)
        assert r["place_tried"] and r["relocalization_tried"] and len(r["place_frames"]) == 2
        if q == len(pc.QUERIES):   # far from every key-frame: nothing is accepted, the request stays
            print("far query: place", r["place_frames"], r["place_dists"], "best quality", r["reloc_best_quality"])
            assert not r["relocalized"] and o.request is not None
            continue
        k, yaw, _ = pc.QUERIES[q]
        full = o.place_search(o.for_map)
        assert full[0][0] == k and full[0][2] < full[1][2]   # the true frame first, strictly
        want = round(-yaw * 64 / (2 * np.pi)) % 64
        assert min((r["place_shifts"][0] - want) % 64, (want - r["place_shifts"][0]) % 64) <= 1   # the shift follows the yaw to a sector
        assert r["relocalized"] and o.request is None
        err = float(np.abs(np.array(r["pose"])[[3, 7, 11]] - pc.query_pose(q)[:3]).max())
        print("query", q, "place", r["place_frames"], r["place_shifts"], r["place_dists"], "quality", r["reloc_best_quality"], "error [m]", err)
        assert err < pc.GT_BOUND
