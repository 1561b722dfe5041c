"""mh_nn_search_radius (every stored map point within a radius of each scan point) against tests/radius_ref.py: a brute force
over all stored points of the oracle's map.  Every comparison is bit for bit -- offsets, global_idx, the float bits of xyz and d2;
there are no tolerances.  tests/test_radius_cpu.py shows on the reference alone what the shared inputs reach."""
import ctypes as C

import numpy as np
import pytest

import lidar2d_inline
import occmap_ref
import radius_ref as rr
from mola_lidar_odometry_amd import capi
from oracle import oracle_c

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"floor": (capi.INDEX_FLOOR, oracle_c.INDEX_FLOOR), "trunc": (capi.INDEX_TRUNC, oracle_c.INDEX_TRUNC)}
INVALID, UNSUPPORTED = 1, 6


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


class _Once:
    """references computed once per module, on first use, and left unchanged"""

    def __init__(self, make):
        self.make, self.done = make, {}

    def __getitem__(self, key):
        if key not in self.done:
            self.done[key] = self.make(key)
        return self.done[key]


@pytest.fixture(scope="module")
def capped(ctx, oracle):
    """mode -> (device map, dump of the oracle's map)"""
    def make(mode):
        return (capi.Map(ctx, 1.0, 20, index_mode=MODES[mode][0]).build(rr.capped_points()),
                oracle_c.Map(1.0, 20, index_mode=MODES[mode][1]).insert(rr.capped_points()).dump())
    return _Once(make)


@pytest.fixture(scope="module")
def capped_scan(ctx):
    return capi.Scan(ctx, rr.capped_queries())


@pytest.fixture(scope="module")
def capped_refs(capped):
    return _Once(lambda k: rr.radius_search(capped[k[0]][1], 1.0, rr.capped_queries(), rr.pose(), k[1], sorted=k[2]))


def _agree(got, ref):
    what = rr.same(got, ref)
    assert what is None, what


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
@pytest.mark.parametrize("radius", rr.RADII)
@pytest.mark.parametrize("mode", list(MODES))
def test_capped_map(capped, capped_scan, capped_refs, mode, radius, sorted_):
    ref = capped_refs[(mode, radius, sorted_)]
    _agree(capi.nn_search_radius(capped[mode][0], capped_scan, rr.pose(), radius, sorted=sorted_), ref)


def test_the_device_map_stores_what_the_oracle_s_does(capped):
    for mode in MODES:
        d, o = capped[mode][0].download(), capped[mode][1]
        assert np.array_equal(d["xyz"].view(np.uint32), o["xyz"].view(np.uint32)) and np.array_equal(d["src_idx"], o["src_idx"])


@pytest.mark.parametrize("radius", [0.5, 1.0])
@pytest.mark.parametrize("mode", list(MODES))
def test_first_sorted_result_is_the_dense_search_s_answer(capped, capped_scan, mode, radius):
    off, gi, xyz, d2 = capi.nn_search_radius(capped[mode][0], capped_scan, rr.pose(), radius, sorted=True)
    dense = capi.nn_search_dense(capped[mode][0], capped_scan, rr.pose())
    within = (dense["global_idx"] != capi.NO_MATCH) & (dense["d2"] < rr.r2_of(radius))
    assert within.sum() > 20 and (np.diff(off.astype(np.int64))[within] > 0).all()
    first = off[:-1][within].astype(np.int64)
    assert np.array_equal(gi[first], dense["global_idx"][within])
    assert np.array_equal(d2[first].view(np.uint32), dense["d2"][within].view(np.uint32))
    assert np.array_equal(xyz[first].view(np.uint32), dense["global_xyz"][within].view(np.uint32))


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
@pytest.mark.parametrize("radius", rr.BOUNDARY_RADII)
@pytest.mark.parametrize("mode", list(MODES))
def test_boundary_points(ctx, oracle, mode, radius, sorted_):
    m = capi.Map(ctx, 1.0, 0, index_mode=MODES[mode][0]).build(rr.boundary_points())
    d = oracle_c.Map(1.0, 0, index_mode=MODES[mode][1]).insert(rr.boundary_points()).dump()
    s = capi.Scan(ctx, rr.boundary_queries())
    ref = rr.radius_search(d, 1.0, rr.boundary_queries(), rr.IDENTITY, radius, sorted=sorted_)
    assert ref.counts().max() > 0
    _agree(capi.nn_search_radius(m, s, rr.IDENTITY, radius, sorted=sorted_), ref)
    m.close()
    s.close()


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
@pytest.mark.parametrize("radius", [0.5, 1.0, 3.0])
def test_dense_uncapped_map(ctx, oracle, radius, sorted_):
    m = capi.Map(ctx, 1.0, 0).build(rr.dense_points())
    d = oracle_c.Map(1.0, 0).insert(rr.dense_points()).dump()
    s = capi.Scan(ctx, rr.dense_queries())
    ref = rr.radius_search(d, 1.0, rr.dense_queries(), rr.pose(), radius, sorted=sorted_)
    assert ref.counts().max() > (256 if radius >= 1.0 else 64)   # rows longer than four 64-record steps / than one
    _agree(capi.nn_search_radius(m, s, rr.pose(), radius, sorted=sorted_), ref)
    m.close()
    s.close()


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
def test_ndt_map_never_returns_a_statistics_record(ctx, oracle, capped_scan, sorted_):
    m = capi.Map(ctx, 1.0, 20, ndt_max_eigen_ratio=0.1).build(rr.capped_points())
    om = oracle_c.Map(1.0, 20, ndt_max_eigen_ratio=0.1).insert(rr.capped_points())
    assert m.info().n_planes == om.dump_ndt()["is_plane"].sum()
    for radius in (0.5, 2.5):
        _agree(capi.nn_search_radius(m, capped_scan, rr.pose(), radius, sorted=sorted_),
               rr.radius_search(om.dump(), 1.0, rr.capped_queries(), rr.pose(), radius, sorted=sorted_))
    m.close()


def test_after_two_queued_inserts(ctx, oracle, capped_scan):
    T2 = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0.125], np.float64)
    m = capi.Map(ctx, 1.0, 20)
    s1, s2 = capi.Scan(ctx, rr.capped_points()), capi.Scan(ctx, rr.second_keyframe())
    m.insert(s1, rr.IDENTITY, 0.0).insert(s2, T2, 3.0)   # (queued: the search orders itself behind them)
    got = capi.nn_search_radius(m, capped_scan, rr.pose(), 1.0)
    om = oracle_c.Map(1.0, 20).insert_posed(rr.capped_points(), rr.IDENTITY, 0.0).insert_posed(rr.second_keyframe(), T2, 3.0)
    kept_all = oracle_c.Map(1.0, 20).insert_posed(rr.capped_points(), rr.IDENTITY, 0.0).insert_posed(rr.second_keyframe(), T2, 0.0)
    assert om.num_points < kept_all.num_points   # the far-voxel removal took something away
    _agree(got, rr.radius_search(om.dump(), 1.0, rr.capped_queries(), rr.pose(), 1.0))
    _agree(capi.nn_search_radius(m, capped_scan, rr.pose(), 2.5, sorted=True),
           rr.radius_search(om.dump(), 1.0, rr.capped_queries(), rr.pose(), 2.5, sorted=True))
    for h in (m, s1, s2):
        h.close()


# ---- the calling protocol, through the raw entry point -------------------------------------------------------------------------
def _raw(m, s, T, radius, flags, out, mem, info):
    T = None if T is None else np.ascontiguousarray(T, np.float64)
    return capi.lib().mh_nn_search_radius(m._h if m is not None else None, s._h if s is not None else None,
                                          T.ctypes.data_as(C.POINTER(C.c_double)) if T is not None else None, float(radius),
                                          int(flags), C.byref(out) if out is not None else None, mem,
                                          C.byref(info) if info is not None else None)


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.mark.parametrize("flags", [capi.RADIUS_VISIT_ORDER, capi.RADIUS_SORTED], ids=["visit", "sorted"])
def test_capacity_protocol(capped, capped_scan, capped_refs, flags):
    m, ref = capped["floor"][0], capped_refs[("floor", 1.0, bool(flags))]
    k, n = len(ref.d2), len(ref.offsets) - 1
    # count only: every array NULL, and no mh_radius_out at all
    for out in (capi.RadiusOut(), None):
        info = capi.RadiusInfo()
        assert _raw(m, capped_scan, rr.pose(), 1.0, flags, out, capi.MEM_HOST, info) == 0
        assert (info.n_results, info.n_written, info.max_per_query) == (k, 0, ref.counts().max())
    # one entry short: offsets and info filled, the result arrays untouched
    off = np.full(n + 1, 0xABABABAB, np.uint32)
    gi = np.full(k, 0xCDCDCDCD, np.uint32)
    fl = [np.full(k, -7.5, F) for _ in range(4)]
    out = capi.RadiusOut(_u32p(off), _u32p(gi), *[_f32p(a) for a in fl], k - 1)
    info = capi.RadiusInfo()
    assert _raw(m, capped_scan, rr.pose(), 1.0, flags, out, capi.MEM_HOST, info) == 0
    assert (info.n_results, info.n_written) == (k, 0) and np.array_equal(off, ref.offsets)
    assert (gi == 0xCDCDCDCD).all() and all((a == F(-7.5)).all() for a in fl)
    # exact capacity
    out.capacity = k
    assert _raw(m, capped_scan, rr.pose(), 1.0, flags, out, capi.MEM_HOST, info) == 0
    assert (info.n_results, info.n_written) == (k, k)
    _agree((off, gi, np.stack(fl[:3], 1), fl[3]), ref)
    # a subset of the arrays
    d2 = np.zeros(k, F)
    out = capi.RadiusOut(None, None, None, None, None, _f32p(d2), k)
    assert _raw(m, capped_scan, rr.pose(), 1.0, flags, out, capi.MEM_HOST, info) == 0
    assert np.array_equal(d2.view(np.uint32), ref.d2.view(np.uint32))


@pytest.mark.parametrize("flags", [capi.RADIUS_VISIT_ORDER, capi.RADIUS_SORTED], ids=["visit", "sorted"])
def test_device_outputs_equal_host_outputs(capped, capped_scan, capped_refs, flags):
    import torch
    m, ref = capped["floor"][0], capped_refs[("floor", 1.0, bool(flags))]
    k, n = len(ref.d2), len(ref.offsets) - 1
    dev = torch.device("cuda:0")
    off, gi = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(k, dtype=torch.int32, device=dev)
    fl = [torch.zeros(k, dtype=torch.float32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    vp = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_uint32 if t.dtype == torch.int32 else C.c_float))  # noqa: E731
    out = capi.RadiusOut(vp(off), vp(gi), *[vp(a) for a in fl], k)
    info = capi.RadiusInfo()
    assert _raw(m, capped_scan, rr.pose(), 1.0, flags, out, capi.MEM_DEVICE, info) == 0
    assert (info.n_results, info.n_written) == (k, k)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    _agree((h(off).view(np.uint32), h(gi).view(np.uint32), np.stack([h(a) for a in fl[:3]], 1), h(fl[3])), ref)


def test_degenerate_queries_give_empty_rows(ctx, capped, capped_refs):
    q = rr.capped_queries()[:40].copy()
    bad = {5: [np.nan, 0, 0], 17: [0, np.inf, 0], 18: [0, 0, -np.inf], 30: [2.0e6, 0, 0]}
    for i, v in bad.items():
        q[i] = v
    s = capi.Scan(ctx, q)
    for sorted_ in (False, True):
        ref_all = capped_refs[("floor", 1.0, sorted_)]
        off, gi, xyz, d2 = capi.nn_search_radius(capped["floor"][0], s, rr.pose(), 1.0, sorted=sorted_)
        c = np.diff(off.astype(np.int64))
        assert (c[list(bad)] == 0).all() and c.sum() > 0
        for i in range(40):
            if i not in bad:   # the neighbours' rows are those of the undisturbed scan
                a, b = slice(int(off[i]), int(off[i + 1])), ref_all.row(i)
                assert np.array_equal(gi[a], ref_all.global_idx[b]) and np.array_equal(d2[a].view(np.uint32), ref_all.d2[b].view(np.uint32))
        _agree((off, gi, xyz, d2), rr.radius_search(capped["floor"][1], 1.0, q, rr.pose(), 1.0, sorted=sorted_))
    s.close()


def test_empty_scan_and_empty_map(ctx, capped, capped_scan):
    s = capi.Scan(ctx)
    off = np.full(1, 77, np.uint32)
    out, info = capi.RadiusOut(), capi.RadiusInfo(9, 9, 9, 9)
    out.offsets = _u32p(off)
    assert _raw(capped["floor"][0], s, rr.IDENTITY, 1.0, 0, out, capi.MEM_HOST, info) == 0
    assert off[0] == 0 and (info.n_results, info.n_written, info.max_per_query) == (0, 0, 0)
    m = capi.Map(ctx, 1.0, 20)
    off, gi, xyz, d2 = capi.nn_search_radius(m, capped_scan, rr.pose(), 1.0)
    assert (off == 0).all() and len(off) == 258 and len(gi) == 0
    m.close()
    s.close()


def test_refusals(ctx, capped, capped_scan):
    m, s, T = capped["floor"][0], capped_scan, rr.pose()
    H = capi.MEM_HOST
    info = capi.RadiusInfo()
    assert _raw(None, s, T, 1.0, 0, None, H, info) == INVALID
    assert _raw(m, None, T, 1.0, 0, None, H, info) == INVALID
    assert _raw(m, s, None, 1.0, 0, None, H, info) == INVALID
    assert _raw(m, s, T, 1.0, 0, None, H, None) == INVALID
    assert _raw(m, s, T, 1.0, 0, None, capi.MEM_HOST_PINNED, info) == INVALID
    assert _raw(m, s, T, 1.0, 0, None, 7, info) == INVALID
    for i in (0, 3, 11):
        Tb = T.copy()
        Tb[i] = np.nan if i else np.inf
        assert _raw(m, s, Tb, 1.0, 0, None, H, info) == INVALID
    for r in (0.0, -1.0, np.nan, np.inf):
        assert _raw(m, s, T, r, 0, None, H, info) == INVALID
    for flags in (2, 3, 0x80000000):
        assert _raw(m, s, T, 1.0, flags, None, H, info) == INVALID
    assert capi.RADIUS_MAX_VOXELS == 3
    assert _raw(m, s, T, 3.0, 0, None, H, info) == 0
    assert _raw(m, s, T, np.nextafter(3.0, 4.0), 0, None, H, info) == UNSUPPORTED
    assert b"MH_RADIUS_MAX_VOXELS" in capi.lib().mh_last_error_string()
    if capi.device_count() > 1:   # a map and a scan on different devices (needs two)
        other = capi.Context(1)
        s1 = capi.Scan(other, rr.capped_queries())
        assert _raw(m, s1, T, 1.0, 0, None, H, info) == INVALID
        other.close()
    # a refused call leaves the handles usable
    assert _raw(m, s, T, 1.0, 0, None, H, info) == 0 and info.n_results > 0


def test_a_total_of_two_to_the_32_results_is_refused(ctx):
    """36 000 stored points in one voxel, 120 000 queries inside it, every pair within the radius: 4.32e9 results.  Only the
    count pass runs: the sum is kept in 64 bits and the call refuses before it sizes anything."""
    rng = np.random.default_rng(1)
    m = capi.Map(ctx, 1.0, 0).build(rng.uniform(0.1, 0.9, (36000, 3)).astype(F))
    s = capi.Scan(ctx, rng.uniform(0.1, 0.9, (120000, 3)).astype(F))
    info = capi.RadiusInfo()
    assert _raw(m, s, rr.IDENTITY, 3.0, 0, None, capi.MEM_HOST, info) == UNSUPPORTED
    assert info.n_results == 36000 * 120000 and info.n_written == 0 and info.max_per_query == 36000
    m.close()
    s.close()


# ---- the host layer --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
def test_host_hashed_voxel_pointcloud(host, capped_refs, sorted_):
    h = host.HashedVoxelPointCloud(1.0, 20)
    h.setPoints(rr.capped_points())
    _agree(h.radiusSearch(rr.capped_queries(), list(rr.pose()), 1.0, sorted_), capped_refs[("floor", 1.0, sorted_)])


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
def test_host_sparse_trees_pointcloud(host, oracle, sorted_):
    h = host.SparseTreesPointCloud(1.0, 0.0)
    h.setPoints(rr.dense_points())
    d = oracle_c.Map(1.0, 0).insert(rr.dense_points()).dump()
    _agree(h.radiusSearch(rr.dense_queries(), list(rr.pose()), 1.0, sorted_),
           rr.radius_search(d, 1.0, rr.dense_queries(), rr.pose(), 1.0, sorted=sorted_))


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
def test_host_voxel_map_answers_over_its_occupied_centres(host, oracle, sorted_):
    _, poses, scans = lidar2d_inline.drive(n_scans=4)
    vm, ref_map = host.CVoxelMap(lidar2d_inline.RESOLUTION), occmap_ref.OccMapRef(resolution=lidar2d_inline.RESOLUTION)
    for T, sc in zip(poses[:3], scans[:3]):
        vm.insertPointCloud(sc, list(T[:3].reshape(12)), 60.0)
        ref_map.insert(sc, T[:3].reshape(12), 60.0)
    centres = ref_map.centres()
    assert vm.size() == len(centres) > 100
    T3, radius = poses[3][:3].reshape(12), 0.12
    got = vm.radiusSearch(scans[3], list(T3), radius, sorted_)
    d = oracle_c.Map(vm.searchVoxelSize(), 0).insert(centres).dump()
    ref = rr.radius_search(d, vm.searchVoxelSize(), scans[3], T3, radius, sorted=sorted_)
    assert ref.counts().max() > 3
    _agree(got, ref)
