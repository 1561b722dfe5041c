"""mh_score_poses (one scan scored under many candidate poses in one launch) against tests/score_ref.py, the restatement on
the CPU oracle's matcher.  Every comparison is bit for bit -- n_paired and the integer cost of every candidate; there are no
tolerances.  A second check is the identity "score == host reduction of capi.nn_search called once per candidate".
tests/test_score_cpu.py shows on the reference alone what the shared inputs reach."""
import ctypes as C

import numpy as np
import pytest

import score_ref as sr
from mola_lidar_odometry_amd import capi, synth
from oracle import oracle_c

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"floor": (capi.INDEX_FLOOR, oracle_c.INDEX_FLOOR), "trunc": (capi.INDEX_TRUNC, oracle_c.INDEX_TRUNC)}
INVALID, UNSUPPORTED = 1, 6
THRESHOLDS = [(0.05, 0.0), (0.5, 0.0), (1.0, 0.0), (0.5, 0.5)]   # (threshold [m], angular threshold [deg])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cube(ctx, oracle):
    """mode -> (device map, oracle map) of the capped cube (voxel 1.0, cap 20; TRUNC's voxel 0 is used)"""
    return {mode: (capi.Map(ctx, 1.0, 20, index_mode=MODES[mode][0]).build(sr.cube_points()),
                   oracle_c.Map(1.0, 20, index_mode=MODES[mode][1]).insert(sr.cube_points())) for mode in MODES}


def _agree(got, ref):
    what = sr.same(got, ref)
    assert what is None, what


def test_the_device_map_stores_what_the_oracle_s_does(cube):
    for mode in MODES:
        d, o = cube[mode][0].download(), cube[mode][1].dump()
        assert np.array_equal(d["xyz"].view(np.uint32), o["xyz"].view(np.uint32)) and np.array_equal(d["src_idx"], o["src_idx"])


@pytest.mark.parametrize("n_scan", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("mode", list(MODES))
def test_scan_sizes_candidate_counts_thresholds(ctx, cube, mode, n_scan):
    """a wave less one, a wave, a wave plus one, a workgroup plus one; 1, 3 and 65 candidates; every threshold"""
    m, om = cube[mode]
    scan = sr.cube_scan(n_scan)
    s = capi.Scan(ctx, scan)
    paired = 0
    for k in (1, 3, 65):
        poses = sr.cube_poses(k, seed=100 + k)
        for thr, ang in THRESHOLDS:
            ref = sr.score_poses(oracle_c, om, scan, poses, thr, ang)
            _agree(capi.score_poses(m, s, poses, thr, ang), ref)
            paired += int(ref["n_paired"].sum())
    assert paired > 0 or n_scan == 1
    s.close()


@pytest.fixture(scope="module")
def small(ctx, oracle):
    w = synth.workload_small()
    poses, rows = sr.small_grid(w)
    om = oracle_c.Map(w.voxel_size, w.cap).insert(w.map_xyz)
    return dict(w=w, poses=poses, rows=rows, om=om, m=capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz),
                s=capi.Scan(ctx, w.scan_xyz), ref=sr.score_poses(oracle_c, om, w.scan_xyz, poses, sr.THRESHOLD))


def test_grid_of_1521_candidates_over_2000_points(small):
    got = capi.score_poses(small["m"], small["s"], small["poses"], sr.THRESHOLD)
    _agree(got, small["ref"])
    assert got["n_paired"].max() == 1661
    assert np.array_equal(sr.rank(got)[:4], sr.rank(small["ref"])[:4])


@pytest.mark.parametrize("thr,ang", [t for t in THRESHOLDS if t != (0.5, 0.0)])
def test_the_other_thresholds_over_2000_points(small, thr, ang):
    poses = small["poses"][400:465]
    _agree(capi.score_poses(small["m"], small["s"], poses, thr, ang),
           sr.score_poses(oracle_c, small["om"], small["w"].scan_xyz, poses, thr, ang))


def test_70000_candidates_cross_the_grid_limit_of_one_dimension(ctx, cube):
    m, om = cube["floor"]
    scan, poses = sr.cube_scan(5, seed=9), sr.cube_poses(70000)
    s = capi.Scan(ctx, scan)
    ref = sr.score_poses(oracle_c, om, scan, poses, 0.5)
    assert ref["n_paired"][65536:].sum() > 1000   # the candidates past 65535 do pair
    _agree(capi.score_poses(m, s, poses, 0.5), ref)
    s.close()


def test_score_is_the_reduction_of_nn_search_per_candidate(ctx, cube):
    m, _ = cube["floor"]
    s = capi.Scan(ctx, sr.cube_scan(257))
    poses = sr.cube_poses(65, seed=3)
    for thr, ang in ((0.5, 0.0), (0.5, 0.5)):
        got = capi.score_poses(m, s, poses, thr, ang)
        for c, T in enumerate(poses):
            n, cost = sr.reduce_pairs(capi.nn_search(m, s, T, thr, ang)["d2"], thr)
            assert (int(got["n_paired"][c]), int(got["cost"][c])) == (n, cost), c
    s.close()


def test_ndt_map_never_pairs_with_a_statistics_record(ctx, oracle):
    m = capi.Map(ctx, 1.0, 20, ndt_max_eigen_ratio=0.1, min_distance_between_points=0.05).build(sr.cube_points())
    om = oracle_c.Map(1.0, 20, ndt_max_eigen_ratio=0.1, min_distance_between_points=0.05).insert(sr.cube_points())
    assert m.info().n_planes == om.dump_ndt()["is_plane"].sum()
    scan, poses = sr.cube_scan(257), sr.cube_poses(65, seed=4)
    s = capi.Scan(ctx, scan)
    for thr, ang in THRESHOLDS:
        _agree(capi.score_poses(m, s, poses, thr, ang), sr.score_poses(oracle_c, om, scan, poses, thr, ang))
    m.close()
    s.close()


def test_uncapped_dense_voxels(ctx, oracle):
    m = capi.Map(ctx, 1.0, 0).build(sr.dense_points())
    om = oracle_c.Map(1.0, 0).insert(sr.dense_points())
    scan = np.random.default_rng(5).uniform(-0.5, 3.5, (257, 3)).astype(F)
    poses = sr.cube_poses(65, seed=6)
    s = capi.Scan(ctx, scan)
    for thr, ang in THRESHOLDS:
        ref = sr.score_poses(oracle_c, om, scan, poses, thr, ang)
        _agree(capi.score_poses(m, s, poses, thr, ang), ref)
    assert ref["n_paired"].max() > 20
    m.close()
    s.close()


def test_empty_map_empty_scan_and_no_poses(ctx, cube):
    m = capi.Map(ctx, 1.0, 20)
    s = capi.Scan(ctx, sr.cube_scan(65))
    got = capi.score_poses(m, s, sr.cube_poses(3), 0.5)
    assert len(got) == 3 and not got["n_paired"].any() and not got["cost"].any()
    e = capi.Scan(ctx)
    out = np.full(3, 0xAB, sr.SCORE_DTYPE)
    P = sr.cube_poses(3)
    assert _raw(cube["floor"][0], e, P, 3, 0.5, 0.0, out, capi.MEM_HOST) == 0
    assert not out["n_paired"].any() and not out["cost"].any() and not out["reserved_"].any()
    out = np.full(3, 0xAB, sr.SCORE_DTYPE)
    assert _raw(cube["floor"][0], s, P, 0, 0.5, 0.0, out, capi.MEM_HOST) == 0 and (out["n_paired"] == 0xAB).all()
    assert _raw(cube["floor"][0], s, None, 0, 0.5, 0.0, out, capi.MEM_HOST) == 0
    for h in (m, s, e):
        h.close()


def test_non_finite_points_far_candidates_and_duplicates(ctx, cube):
    m, om = cube["floor"]
    scan = sr.cube_scan(130, seed=21)
    for i, v in {5: [np.nan, 0, 0], 64: [0, np.inf, 0], 65: [0, 0, -np.inf], 129: [np.nan, np.nan, np.nan]}.items():
        scan[i] = v
    poses = sr.cube_poses(4, seed=8)
    poses[1] = synth.pose_from_ypr([2.0e6, 0.0, 0.0, 0.1, 0.0, 0.0])   # beyond the key range: pairs with nothing
    poses[3] = poses[0]                                                 # identical candidates: identical scores
    s = capi.Scan(ctx, scan)
    got = capi.score_poses(m, s, poses, 0.5)
    _agree(got, sr.score_poses(oracle_c, om, scan, poses, 0.5))
    assert (got["n_paired"][1], got["cost"][1]) == (0, 0) and got[0] == got[3] and got["n_paired"][0] > 0
    # the undisturbed points pair as they do without the non-finite ones
    keep = np.ones(130, bool)
    keep[[5, 64, 65, 129]] = False
    s2 = capi.Scan(ctx, scan[keep])
    _agree(capi.score_poses(m, s2, poses, 0.5), got)
    s.close()
    s2.close()


def test_quantised_residual_saturates(ctx, oracle):
    """threshold 0.5: qscale = 2^22, so d2 >= 4 saturates; a 10 deg angular threshold accepts such a pair 19 m from the origin"""
    pts = np.array([[20.99, 0.99, 0.99], [0.5, 0.5, 0.5]], F)
    scan = np.array([[19.01, 0.01, 0.01], [0.4, 0.5, 0.5], [17.5, 0.2, 0.2]], F)   # saturated, plain, unpaired
    m, om = capi.Map(ctx, 1.0, 20).build(pts), oracle_c.Map(1.0, 20).insert(pts)
    s = capi.Scan(ctx, scan[:1])
    I = synth.pose_from_ypr([0, 0, 0, 0, 0, 0])
    got = capi.score_poses(m, s, [I], 0.5, 10.0)
    assert (int(got["n_paired"][0]), int(got["cost"][0])) == (1, 0xFFFFFF)   # the pair at d2 = 5.84
    _agree(got, sr.score_poses(oracle_c, om, scan[:1], [I], 0.5, 10.0))
    s3 = capi.Scan(ctx, scan)
    _agree(capi.score_poses(m, s3, [I, I], 0.5, 10.0), sr.score_poses(oracle_c, om, scan, [I, I], 0.5, 10.0))
    for h in (m, s, s3):
        h.close()


def test_device_scores_equal_host_scores_and_runs_repeat(small):
    import torch
    k = 65
    poses = np.ascontiguousarray(small["poses"][400:400 + k])
    host = capi.score_poses(small["m"], small["s"], poses, 0.5)
    again = capi.score_poses(small["m"], small["s"], poses, 0.5)
    assert host.tobytes() == again.tobytes()   # two calls, the same bits
    dev = torch.full((k, 2), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st = capi.lib().mh_score_poses(small["m"]._h, small["s"]._h, poses.ctypes.data_as(C.POINTER(C.c_double)), k, 0.5, 0.0,
                                   C.c_void_p(dev.data_ptr()), capi.MEM_DEVICE)
    assert st == 0
    assert dev.cpu().numpy().tobytes() == host.tobytes()
    _agree(host, small["ref"][400:400 + k])


def test_a_call_queued_behind_an_insert_sees_the_inserted_points(ctx, oracle):
    T2 = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0.125], np.float64)
    I = synth.pose_from_ypr([0, 0, 0, 0, 0, 0])
    second = np.random.default_rng(11).uniform(-2.0, 5.0, (1500, 3)).astype(F)
    scan, poses = sr.cube_scan(257), sr.cube_poses(65, seed=12)
    m = capi.Map(ctx, 1.0, 20)
    s1, s2, s = capi.Scan(ctx, sr.cube_points()), capi.Scan(ctx, second), capi.Scan(ctx, scan)
    m.insert(s1, I, 0.0).insert(s2, T2, 3.0)   # (queued: the call orders itself behind them)
    queued = capi.score_poses(m, s, poses, 0.5)
    ctx.synchronize()
    assert capi.score_poses(m, s, poses, 0.5).tobytes() == queued.tobytes()
    om = oracle_c.Map(1.0, 20).insert_posed(sr.cube_points(), I, 0.0).insert_posed(second, T2, 3.0)
    _agree(queued, sr.score_poses(oracle_c, om, scan, poses, 0.5))
    for h in (m, s1, s2, s):
        h.close()


# ---- the calling protocol, through the raw entry point -------------------------------------------------------------------------
def _raw(m, s, poses, n_poses, thr, ang, out, mem):
    P = None if poses is None else np.ascontiguousarray(poses, np.float64)
    return capi.lib().mh_score_poses(m._h if m is not None else None, s._h if s is not None else None,
                                     P.ctypes.data_as(C.POINTER(C.c_double)) if P is not None else None, n_poses, float(thr),
                                     float(ang), out.ctypes.data_as(C.c_void_p) if out is not None else None, mem)


def test_refusals(ctx, cube):
    m = cube["floor"][0]
    s = capi.Scan(ctx, sr.cube_scan(65))
    P, H = sr.cube_poses(3), capi.MEM_HOST
    out = np.zeros(3, sr.SCORE_DTYPE)
    assert _raw(None, s, P, 3, 0.5, 0.0, out, H) == INVALID
    assert _raw(m, None, P, 3, 0.5, 0.0, out, H) == INVALID
    assert _raw(m, s, None, 3, 0.5, 0.0, out, H) == INVALID
    assert _raw(m, s, P, 3, 0.5, 0.0, None, H) == INVALID
    assert _raw(m, s, P, 3, 0.5, 0.0, out, capi.MEM_HOST_PINNED) == INVALID
    assert _raw(m, s, P, 3, 0.5, 0.0, out, 7) == INVALID
    for c, i, v in ((0, 0, np.inf), (1, 3, np.nan), (2, 11, -np.inf)):
        Pb = P.copy()
        Pb[c, i] = v
        assert _raw(m, s, Pb, 3, 0.5, 0.0, out, H) == INVALID
    for thr in (np.nan, np.inf, 0.0, -0.5, np.nextafter(1e-3, 0.0), np.nextafter(1e3, 2e3)):
        assert _raw(m, s, P, 3, thr, 0.0, out, H) == INVALID
    for thr in (1e-3, 1e3):
        assert _raw(m, s, P, 3, thr, 0.0, out, H) == 0
    for ang in (-1.0, np.nan, np.inf):
        assert _raw(m, s, P, 3, 0.5, ang, out, H) == INVALID
    assert capi.SCORE_MAX_POSES == 1 << 20
    assert _raw(m, s, P, (1 << 20) + 1, 0.5, 0.0, out, H) == UNSUPPORTED   # (refused before a pose is read)
    assert b"MH_SCORE_MAX_POSES" in capi.lib().mh_last_error_string()
    if capi.device_count() > 1:   # a map and a scan on different devices (needs two)
        other = capi.Context(1)
        s1 = capi.Scan(other, sr.cube_scan(65))
        assert _raw(m, s1, P, 3, 0.5, 0.0, out, H) == INVALID
        other.close()
    # a refused call leaves the handles usable
    assert _raw(m, s, P, 3, 0.5, 0.0, out, H) == 0 and out["n_paired"].sum() > 0
    s.close()
