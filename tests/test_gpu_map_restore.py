"""mh_map_restore: a map downloaded and restored into a fresh handle is indistinguishable from the original -- downloads, NDT
statistics, counts, every search route, an alignment and a following insertion, all bit for bit.  The originals are built by a
build plus three insertions with far-voxel removal and are held to the CPU oracle's dump first."""
import ctypes as C

import numpy as np
import pytest

import score_ref as sr
from mola_lidar_odometry_amd import capi, synth
from oracle import oracle_c

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = 1
FAR = 4.0
KINDS = {
    "capped_floor": dict(voxel_size=1.0, max_points_per_voxel=20, index_mode="floor"),
    "capped_trunc": dict(voxel_size=1.0, max_points_per_voxel=20, index_mode="trunc"),
    "ndt": dict(voxel_size=1.0, max_points_per_voxel=20, index_mode="floor", ndt_max_eigen_ratio=0.1,
                min_distance_between_points=0.05),
    "uncapped": dict(voxel_size=1.0, max_points_per_voxel=0, index_mode="floor"),
}
IDX = {"floor": (capi.INDEX_FLOOR, oracle_c.INDEX_FLOOR), "trunc": (capi.INDEX_TRUNC, oracle_c.INDEX_TRUNC)}


def _params(kind, which):
    p = dict(KINDS[kind])
    p["index_mode"] = IDX[p["index_mode"]][which]
    return p


def _first_points(kind):
    return sr.dense_points() if kind == "uncapped" else sr.cube_points()


def _keyframes(kind):
    """three (layer, pose) pairs: the vehicle moves 1.5 m along x per key-frame, so the far-voxel removal takes voxels away"""
    out = []
    for j in range(4):
        rng = np.random.default_rng(40 + j)
        if kind == "uncapped":   # more records for the dense voxels, and some new voxels
            layer = np.concatenate([rng.uniform(0.01, 0.99, (150, 3)) + np.array([j % 3, 0, 0]), rng.uniform(-2, 3, (200, 3))]).astype(F)
        else:
            layer = rng.uniform(-3.0, 3.0, (1500, 3)).astype(F)
        out.append((layer, synth.pose_from_ypr([1.5 * (j + 1), -0.4 * j, 0.1, 0.05 * j, 0.01, -0.02])))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def originals(ctx, oracle):
    """kind -> (device map after build + three insertions, its download, its info, the oracle's map)"""
    done = {}

    def get(kind):
        if kind not in done:
            m = capi.Map(ctx, **_params(kind, 0)).build(_first_points(kind))
            om = oracle_c.Map(**_params(kind, 1)).insert(_first_points(kind))
            for layer, T in _keyframes(kind)[:3]:
                sc = capi.Scan(ctx, layer)
                m.insert(sc, T, FAR)
                sc.close()
                om.insert_posed(layer, T, FAR)
            done[kind] = (m, m.download(), m.info(), om)
        return done[kind]
    return get


def _same_download(a, b):
    for k in ("xyz", "src_idx", "vox_keys", "vox_first", "vox_count"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _same_ndt(a, b):
    for k in ("centroid", "normal", "is_plane"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _info_tuple(i):
    return (i.n_points, i.n_offered, i.n_voxels, i.n_planes, tuple(F(v).tobytes() for v in i.bbox_min),
            tuple(F(v).tobytes() for v in i.bbox_max), i.voxel_size, i.max_points_per_voxel, i.deferred_status)


def _restored(ctx, kind, originals):
    m, d, info, _ = originals(kind)
    return capi.Map(ctx, **_params(kind, 0)).restore(d["xyz"], d["src_idx"], info.n_offered)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_original_is_the_oracle_s_map(originals, kind):
    m, d, info, om = originals(kind)
    o = om.dump()
    assert len(o["xyz"]) > 1000
    for k in ("xyz", "src_idx", "vox_keys", "vox_count"):
        assert d[k].tobytes() == o[k].tobytes(), k
    if kind == "ndt":
        _same_ndt(m.download_ndt(), om.dump_ndt())
        assert info.n_planes > 0
    if kind == "uncapped":
        assert d["vox_count"].max() > 31
    # the far-voxel removal took something away, and the cap was met
    assert info.n_points < info.n_offered
    if KINDS[kind]["max_points_per_voxel"]:
        assert d["vox_count"].max() == 20


@pytest.mark.parametrize("kind", list(KINDS))
def test_restored_map_is_indistinguishable(ctx, originals, kind):
    m, d, info, _ = originals(kind)
    r = _restored(ctx, kind, originals)
    _same_download(r.download(), d)
    _same_ndt(r.download_ndt(), m.download_ndt())
    assert _info_tuple(r.info()) == _info_tuple(info)
    # every search route
    q = capi.Scan(ctx, sr.cube_scan(257, seed=77) if kind != "uncapped" else np.random.default_rng(5).uniform(-0.5, 3.5, (257, 3)).astype(F))
    T = sr.pose(yaw=0.1, t=(2.0, -0.3, 0.05))
    for route in (lambda mm: capi.nn_search_dense(mm, q, T), lambda mm: capi.nn_search(mm, q, T, 0.7),
                  lambda mm: capi.nn_search_k(mm, q, T, 1.0, 3)):
        a, b = route(m), route(r)
        assert (a["global_idx"] != capi.NO_MATCH).sum() > 20
        for k in ("global_idx", "global_xyz", "d2"):
            assert a[k].tobytes() == b[k].tobytes(), k
    for sorted_ in (False, True):
        a, b = capi.nn_search_radius(m, q, T, 1.0, sorted=sorted_), capi.nn_search_radius(r, q, T, 1.0, sorted=sorted_)
        assert len(a[1]) > 100 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # a 20-iteration alignment
    thr, kp = synth.threshold_schedule(2.0, 20)
    p = capi.ICPParams(max_iterations=20, disable_stall_test=True, threshold=thr, kernel_param=kp)
    a, b = capi.icp_align(m, q, T, p), capi.icp_align(r, q, T, p)
    assert a["n_iterations"] == b["n_iterations"] > 0 and a["n_final_pairs"] == b["n_final_pairs"] > 20
    assert np.asarray(a["T"]).tobytes() == np.asarray(b["T"]).tobytes()
    q.close()
    r.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_more_insertion_into_both_gives_the_same_map(ctx, originals, kind):
    """(on copies: the originals stay as the other tests expect them) source indices continue from n_offered, the cap and the
    clearance rule see the restored points as stored ones"""
    a, b = _restored(ctx, kind, originals), _restored(ctx, kind, originals)
    _, d, info, om = originals(kind)
    layer, T = _keyframes(kind)[3]
    sc = capi.Scan(ctx, layer)
    a.insert(sc, T, FAR)
    da = a.download()
    # the oracle's map continues the same way: the restored map inserts as the original would have
    ref = oracle_c.Map(**_params(kind, 1)).insert(_first_points(kind))
    for l, Tk in _keyframes(kind):
        ref.insert_posed(l, Tk, FAR)
    o = ref.dump()
    for k in ("xyz", "src_idx", "vox_keys", "vox_count"):
        assert da[k].tobytes() == o[k].tobytes(), k
    assert da["src_idx"].max() >= info.n_offered and a.info().n_offered == info.n_offered + len(layer)
    # ... and a restore of a restore's download is the same map again
    b.restore(d["xyz"], d["src_idx"], info.n_offered).insert(sc, T, FAR)
    _same_download(b.download(), da)
    for h in (a, b, sc):
        h.close()


def test_empty_restore_keeps_n_offered(ctx):
    m = capi.Map(ctx, 1.0, 20).build(sr.cube_points(500))
    m.restore(np.zeros((0, 3), F), np.zeros(0, np.uint32), 1234)
    i = m.info()
    assert (i.n_points, i.n_voxels, i.n_offered) == (0, 0, 1234)
    assert capi.lib().mh_map_restore(m._h, None, None, None, None, 0, 77, capi.MEM_HOST) == 0 and m.info().n_offered == 77
    sc = capi.Scan(ctx, sr.cube_points(100, seed=2))
    m.insert(sc, synth.pose_from_ypr([0, 0, 0, 0, 0, 0]), 0.0)
    d = m.download()
    assert len(d["src_idx"]) > 0 and d["src_idx"].min() >= 77 and sorted(d["src_idx"]) == list(range(77, 177))
    m.close()
    sc.close()


def test_device_resident_input(ctx, originals):
    import torch
    m, d, info, _ = originals("capped_floor")
    t = [torch.from_numpy(np.ascontiguousarray(d["xyz"][:, a])).to("cuda:0") for a in range(3)]
    src = torch.from_numpy(d["src_idx"].astype(np.int64)).to("cuda:0").to(torch.int32)   # (the indices fit 31 bits here)
    torch.cuda.synchronize()
    r = capi.Map(ctx, **_params("capped_floor", 0))
    r.restore_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), src.data_ptr(), len(d["src_idx"]), info.n_offered)
    _same_download(r.download(), d)
    assert _info_tuple(r.info()) == _info_tuple(info)
    r.close()


def _raw(m, xyz, src, n_offered, n=None):
    x, y, z = (np.ascontiguousarray(xyz[:, a], F) for a in range(3))
    src = np.ascontiguousarray(src, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return capi.lib().mh_map_restore(m._h, vp(x), vp(y), vp(z), vp(src), len(x) if n is None else n, int(n_offered), capi.MEM_HOST)


def _is_empty(ctx, m):
    i = m.info()
    q = capi.Scan(ctx, sr.cube_scan(65))
    none = (capi.nn_search_dense(m, q, sr.pose())["global_idx"] == capi.NO_MATCH).all()
    q.close()
    return (i.n_points, i.n_voxels, i.n_offered, i.deferred_status) == (0, 0, 0, 0) and len(m.download()["xyz"]) == 0 and none


@pytest.mark.parametrize("kind", ["capped_floor", "capped_trunc"])
def test_refusals_leave_the_map_empty(ctx, originals, kind):
    _, d, info, _ = originals(kind)
    xyz, src, first, count = d["xyz"], d["src_idx"], d["vox_first"], d["vox_count"]
    m = capi.Map(ctx, **_params(kind, 0))

    def refused(xyz_, src_, n_offered):
        m.build(sr.cube_points(200))   # something to lose
        st = _raw(m, xyz_, src_, n_offered)
        return st == INVALID and _is_empty(ctx, m)

    # the undisturbed download is accepted
    assert _raw(m, xyz, src, info.n_offered) == 0 and m.info().n_points == info.n_points
    # one swapped pair of voxels
    v = len(count) // 2
    a, b = slice(first[v], first[v] + count[v]), slice(first[v + 1], first[v + 1] + count[v + 1])
    order = np.concatenate([np.arange(0, a.start), np.arange(b.start, b.stop), np.arange(a.start, a.stop), np.arange(b.stop, len(src))])
    assert refused(xyz[order], src[order], info.n_offered)
    assert b"order" in capi.lib().mh_last_error_string()
    # one voxel over the cap: a 21st point in a full voxel
    full = int(np.flatnonzero(count == 20)[0])
    at = int(first[full] + 20)
    assert refused(np.insert(xyz, at, xyz[at - 1], axis=0), np.insert(src, at, src[at - 1]), info.n_offered + 1)
    assert b"max_points_per_voxel" in capi.lib().mh_last_error_string()
    # a NaN, an infinity, a point outside the key range
    for bad in (np.nan, np.inf, 2.0e6):
        x2 = xyz.copy()
        x2[len(x2) // 3, 1] = bad
        assert refused(x2, src, info.n_offered)
    # fewer points offered than stored
    assert refused(xyz, src, len(src) - 1)
    # the wrong index mode or voxel size: the keys are not in order under the map's own parameters
    other = capi.Map(ctx, 0.37, 20, index_mode=IDX["floor"][0])
    assert _raw(other, xyz, src, info.n_offered) == INVALID and other.info().n_points == 0
    # a refused map is usable: the good input is accepted again
    assert _raw(m, xyz, src, info.n_offered) == 0
    _same_download(m.download(), d)
    # NULL arrays with n > 0, a bad mem, a NULL map: refused, and the map is not touched
    L = capi.lib()
    assert L.mh_map_restore(m._h, None, None, None, None, 5, 5, capi.MEM_HOST) == INVALID
    assert L.mh_map_restore(None, None, None, None, None, 0, 0, capi.MEM_HOST) == INVALID
    assert L.mh_map_restore(m._h, None, None, None, None, 0, 0, 7) == INVALID
    assert m.info().n_points == info.n_points
    m.close()
    other.close()
