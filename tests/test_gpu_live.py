"""Erasing moving objects from a live map on the device (include/molahip_live.h) against tests/clean_ref.py, the numpy
restatement of the vote, and against the header's own definition of erasing: a fresh map after mh_map_restore of the download
minus the dropped records.  Every word of every view and vote, every bit of every download.  Small shapes: the largest map
holds about 5 000 points."""
import ctypes as C
import gc

import numpy as np
import pytest

import clean_ref as cr

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 8), (32, 128), (5, 24), (16, 256)]   # 32 x 128 and 16 x 256 fill the 4096 bins a view may have
SCAN_SIZES = [0, 1, 63, 64, 65, 5000]
MAP_KINDS = {  # capi.Map arguments behind the context
    "capped": dict(voxel_size=1.0, max_points_per_voxel=20),
    "clearance": dict(voxel_size=1.0, max_points_per_voxel=0, min_distance_between_points=0.15),
    "ndt": dict(voxel_size=2.0, max_points_per_voxel=0, min_distance_between_points=0.05, ndt_max_eigen_ratio=0.05),
}
I12 = np.eye(4)[:3].reshape(12)


@pytest.fixture(scope="module")
def capi():
    from mola_lidar_odometry_amd import capi as c
    return c


@pytest.fixture(scope="module")
def cl():
    from mola_lidar_odometry_amd import capi_clean
    return capi_clean


@pytest.fixture(scope="module")
def lv():
    from mola_lidar_odometry_amd import capi_live
    return capi_live


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def _params(A, S, **kw):
    p = dict(cr.DEFAULT, n_rings=A, n_sectors=S)
    if A == 5:  # one shape with the sensor off the vehicle's origin and a window that straddles no zero edge
        p.update(origin=(0.25, -0.5, 1.0), el_min=float(np.radians(-30.0)), el_max=float(np.radians(-1.0)))
    if A == 1:
        p.update(el_min=float(np.radians(-10.0)), el_max=float(np.radians(10.0)))
    p.update(kw)
    return p


def _pose(rng, spread):
    yaw = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    t = rng.uniform(-spread, spread, 3) * [1, 1, 0.05]
    return np.array([c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]])


def _shell(p, n, r0, r1, seed):
    """a dense shell around the sensor: every bin of the elevation window holds points"""
    rng = np.random.default_rng(seed)
    e0, e1 = float(F(p["el_min"])), float(F(p["el_max"]))
    az, el, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(e0, e1, n), rng.uniform(r0, r1, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)
    return np.ascontiguousarray((xyz + np.asarray(p["origin"])).astype(F))


def _world(n, seed, lo=-40.0, hi=40.0):
    """n finite points spread over the street's surroundings; (almost) every one in a voxel of its own"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.uniform(lo, hi, (n, 3)) * [1, 1, 0.08]).astype(F))


def _dense(n, seed):
    """n points crowded into a few dozen voxels: caps fill, clearance rejects, NDT voxels find planes"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-6.0, 6.0, (n, 2))
    z = 0.02 * rng.standard_normal(n) + np.where(rng.random(n) < 0.2, rng.uniform(0, 3.0, n), 0.0)
    return np.ascontiguousarray(np.column_stack([xy, z]).astype(F))


def _same_download(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _info(m):
    i = m.info()
    return (int(i.n_points), int(i.n_offered), int(i.n_voxels), tuple(i.bbox_min), tuple(i.bbox_max), int(i.n_planes),
            int(i.deferred_status))


def _twin(capi, ctx, kind, d, n_offered, keep=None):
    """a fresh map of the same parameters after mh_map_restore of (the download minus the dropped records, n_offered)"""
    keep = np.ones(len(d["xyz"]), bool) if keep is None else keep
    return capi.Map(ctx, **MAP_KINDS[kind]).restore(d["xyz"][keep], d["src_idx"][keep], n_offered)


# ------------------------------------------------------------------ mh_views_put_scan
@pytest.mark.parametrize("A,S", SHAPES)
def test_put_scan_writes_the_restatement_s_view_and_add_frames_words(capi, cl, lv, ctx, A, S):
    p = _params(A, S)
    clouds = [cr.edge_cloud(n, 40 + n, **p) for n in SCAN_SIZES] + [cr.edge_cloud(700, 7, **p)]
    ref = np.array([cr.view(c, **p) for c in clouds])
    by_frames = cl.Views(ctx, cl.clean_params(**p)).add_frames(clouds).download()
    v = cl.Views(ctx, cl.clean_params(**p))
    scans = [capi.Scan(ctx, c) for c in clouds]
    for k, s in enumerate(scans):          # slot == size appends
        assert len(v) == k
        lv.put_scan(v, k, s)
    got = v.download()
    assert len(v) == len(clouds) and got.tobytes() == ref.tobytes(), np.argwhere(got != ref)[:5]
    assert got.tobytes() == by_frames.tobytes()
    assert (got[0] == cr.EMPTY).all()      # an empty scan: an all-empty view
    if A > 1:
        assert (got[5] != cr.EMPTY).sum() > A * S // 4
    lv.put_scan(v, 2, scans[5])            # slot < size overwrites, and nothing else moves
    lv.put_scan(v, 5, scans[0])
    again = v.download()
    want = ref.copy()
    want[2], want[5] = ref[5], ref[0]
    assert len(v) == len(clouds) and again.tobytes() == want.tobytes()
    with pytest.raises(capi.MolahipError) as e:   # slot > size
        lv.put_scan(v, len(clouds) + 1, scans[1])
    assert e.value.status == 1 and len(v) == len(clouds) and v.download().tobytes() == want.tobytes()
    other = capi.Context(0)
    with pytest.raises(capi.MolahipError) as e:   # a scan of another context
        lv.put_scan(v, 0, capi.Scan(other, clouds[1]))
    assert e.value.status == 1
    other.close()
    v.close()


# ------------------------------------------------------------------ mh_views_vote_map
def _store(cl, ctx, p, seed):
    stored = [cr.edge_cloud(n, seed + n, **p) for n in (255, 5000)] + [_shell(p, 30000, 8.0, 12.0, seed + 1), _shell(p, 30000, 30.0, 40.0, seed + 2)]
    return cl.Views(ctx, cl.clean_params(**p)).add_frames(stored), [cr.view(f, **p) for f in stored]


def _nbr(rng, n_views, k, spread=6.0):
    view = rng.integers(0, n_views, k).astype(np.uint32)
    if k >= 2:
        view[1] = view[0]   # a view may repeat
    return view, np.array([_pose(rng, spread) for _ in range(k)]).reshape(k, 12)


@pytest.mark.parametrize("n_points", [0, 1, 255, 256, 257, 5000])
def test_votes_on_a_capped_map_are_the_restatement_s_word_for_word(capi, cl, lv, ctx, n_points):
    p = _params(32, 128, win_rings=1, win_sectors=1)
    v, views = _store(cl, ctx, p, 300)
    m = capi.Map(ctx, **MAP_KINDS["capped"]).build(_world(n_points, 11 + n_points))
    xyz = m.download()["xyz"]
    assert len(xyz) == n_points == int(m.info().n_points)   # (one workgroup, its edge, the first lane of a second)
    rng = np.random.default_rng(n_points)
    for k in (0, 1, 24, 64):
        nv, nT = _nbr(rng, len(views), k)
        got = lv.vote_map(v, m, nv, nT)
        ref = cr.vote(xyz, views, nv, nT, **p)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (k, np.argwhere(got != ref)[:5])
        if k == 0:
            assert not got.any()
        if k == 64 and n_points == 5000:
            assert (got & 0xFFFF).max() >= 2 and (got >> 16).max() >= 2   # (the comparison is of counted votes)
    v.close()
    m.close()


@pytest.mark.parametrize("kind", sorted(MAP_KINDS))
@pytest.mark.parametrize("A,S,wr,ws", [(32, 128, 0, 0), (32, 128, 2, 2), (32, 128, 0, 2), (1, 8, 1, 1), (5, 24, 1, 2), (16, 256, 2, 1)])
def test_votes_are_the_restatement_s_on_every_map_kind_shape_and_window(capi, cl, lv, ctx, kind, A, S, wr, ws):
    p = _params(A, S, win_rings=wr, win_sectors=ws)
    v, views = _store(cl, ctx, p, 500 + A)
    m = capi.Map(ctx, **MAP_KINDS[kind])
    m.insert(capi.Scan(ctx, _world(3000, 21)), I12)
    m.insert(capi.Scan(ctx, _dense(3000, 22)), _pose(np.random.default_rng(3), 2.0))
    xyz = m.download()["xyz"]
    assert 3000 < len(xyz) <= 6000
    rng = np.random.default_rng(A + wr)
    nv, nT = _nbr(rng, len(views), 24)
    got = lv.vote_map(v, m, nv, nT, capacity=len(xyz) + 3)   # (room to spare is fine)
    ref = cr.vote(xyz, views, nv, nT, **p)
    assert got.tobytes() == ref.tobytes(), np.argwhere(got != ref)[:5]
    if A > 1:
        assert (got & 0xFFFF).any() and (got >> 16).any()
    # the device destination gets the same words
    import torch
    buf = torch.zeros(len(xyz), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    lv.vote_map_device(v, m, nv, nT, buf.data_ptr(), len(xyz))
    assert buf.cpu().numpy().view(np.uint32).tobytes() == ref.tobytes()
    v.close()
    m.close()


def test_points_exactly_on_the_margin(capi, cl, lv, ctx):
    """rel_margin = 1: far2 = 4 exactly, so squared ranges 64 / 256 / 1024 sit exactly on the two limits of the vote."""
    p = _params(32, 128, rel_margin=1.0, win_rings=0, win_sectors=0)
    up = float(np.nextafter(F(16), F(np.inf)))
    scans = [np.array([[16, 0, 0]], F), np.array([[up, 0, 0]], F), np.array([[8, 0, 0]], F)]
    v = cl.Views(ctx, cl.clean_params(**p))
    for k, s in enumerate(scans):
        lv.put_scan(v, k, capi.Scan(ctx, s))
    views = [cr.view(s, **p) for s in scans]
    m = capi.Map(ctx, **MAP_KINDS["capped"]).build(np.array([[8, 0, 0], [16, 0, 0], [up, 0, 0], [4, 0, 0]], F))
    xyz = m.download()["xyz"]
    words = {}
    for k in range(3):
        got = lv.vote_map(v, m, [k], [I12])
        assert got.tobytes() == cr.vote(xyz, views, [k], [I12], **p).tobytes()
        for pt, w in zip(xyz, got):
            words[(float(pt[0]), k)] = int(w)
    assert words[(8.0, 0)] == 1 << 16      # r2_img == r2_q * far2: not farther, agrees
    assert words[(8.0, 1)] == 1            # one ulp beyond: seen through
    assert words[(16.0, 2)] == 1 << 16     # r2_q == r2_img * far2: still agrees
    assert words[(up, 2)] == 0             # one ulp beyond: occluded, no evidence
    assert words[(4.0, 2)] == 1 << 16 and words[(4.0, 0)] == 1
    v.close()
    m.close()


def test_vote_map_refusals(capi, cl, lv, ctx):
    p = _params(32, 128)
    v = cl.Views(ctx, cl.clean_params(**p)).add_frames([cr.edge_cloud(300, 1, **p)] * 2)
    m = capi.Map(ctx, **MAP_KINDS["capped"]).build(_world(100, 5))
    L, n = lv.lib(), 100
    out = np.full(n, 0xABCDABCD, np.uint32)
    view = np.zeros(65, np.uint32)
    T = np.tile(I12, 65)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(views=v._h, map_=m._h, k=2, nv=view, nT=T, o=out, cap=n, mem=capi.MEM_HOST):
        return L.mh_views_vote_map(views, map_, k, None if nv is None else vp(nv), None if nT is None else vp(nT),
                                   None if o is None else vp(o), cap, mem)

    assert call() == 0 and (out == (2 << 16)).sum() + (out == 0).sum() + (out == 2).sum() == n
    out[:] = 0xABCDABCD
    assert call(views=None) == 1 and call(map_=None) == 1
    assert call(cap=n - 1) == 1                      # capacity below the stored count
    assert call(nv=np.array([0, 2], np.uint32)) == 1   # a neighbour index beyond the store
    for bad in (np.nan, np.inf):
        Tb = T.copy()
        Tb[12 + 7] = bad
        assert call(nT=Tb) == 1                      # a non-finite pose entry
    assert call(k=65) == 1                           # more than MH_LIVE_MAX_VIEWS
    assert call(nv=None) == 1 and call(nT=None) == 1 and call(o=None) == 1
    assert call(mem=7) == 1
    other = capi.Context(0)
    m2 = capi.Map(other, **MAP_KINDS["capped"]).build(_world(100, 5))
    assert call(map_=m2._h) == 1                     # a map and views of different contexts
    assert L.mh_map_erase_seen_through(m2._h, v._h, 1, vp(view), vp(T), 2, 1) == 1
    other.close()
    assert (out == 0xABCDABCD).all()                 # every refusal came before any device work
    assert call(k=64) == 0 and call(k=0, nv=None, nT=None) == 0 and not out.any()
    v.close()
    m.close()


# ------------------------------------------------------------------ mh_map_erase_points
def _filled(capi, ctx, kind):
    m = capi.Map(ctx, **MAP_KINDS[kind])
    m.insert(capi.Scan(ctx, _world(2500, 31)), I12)
    m.insert(capi.Scan(ctx, _dense(2500, 32)), I12)
    m.insert(capi.Scan(ctx, _dense(1500, 33)), _pose(np.random.default_rng(4), 1.0))
    return m


def _patterns(d):
    n = len(d["xyz"])
    first, count = d["vox_first"].astype(np.int64), d["vox_count"].astype(np.int64)
    big = int(np.argmax(count))
    assert count[big] >= 3
    out = dict(none=np.zeros(n, bool), all=np.ones(n, bool), every_other=np.arange(n) % 2 == 0)
    whole = np.zeros(n, bool)
    whole[first[big]:first[big] + count[big]] = True
    ends = np.zeros(n, bool)
    ends[[first[big], first[big] + count[big] - 1]] = True
    out.update(one_whole_voxel=whole, first_and_last_of_a_voxel=ends, the_map_s_first_and_last=np.isin(np.arange(n), [0, n - 1]))
    return out


@pytest.mark.parametrize("kind", sorted(MAP_KINDS))
def test_erase_points_leaves_the_restore_defined_twin(capi, lv, ctx, kind):
    src_map = _filled(capi, ctx, kind)
    d, n_off = src_map.download(), int(src_map.info().n_offered)
    ndt0 = src_map.download_ndt()
    queries = capi.Scan(ctx, np.concatenate([_dense(400, 51), _world(200, 52)]))
    nxt = capi.Scan(ctx, _dense(1200, 53))
    T_next = np.array([1, 0, 0, 1.5, 0, 1, 0, -0.5, 0, 0, 1, 0.0])
    for name, drop in _patterns(d).items():
        m = _twin(capi, ctx, kind, d, n_off)
        _same_download(m.download(), d)
        before = lv.erased_total(m)
        lv.erase_points(m, drop)
        twin = _twin(capi, ctx, kind, d, n_off, ~drop)
        got, want = m.download(), twin.download()
        _same_download(got, want)
        assert got["src_idx"].tobytes() == d["src_idx"][~drop].tobytes(), name   # the source indices are kept
        _same_download(m.download_ndt(), twin.download_ndt())
        assert _info(m) == _info(twin), name
        assert lv.erased_total(m) - before == int(drop.sum())
        if name == "none":   # all zeros: every bit as it was
            _same_download(got, d)
            _same_download(m.download_ndt(), ndt0)
        if name == "one_whole_voxel":   # a voxel that loses its last point is gone
            assert len(got["vox_keys"]) == len(d["vox_keys"]) - 1
        if name == "all":
            assert int(m.info().n_points) == 0 and int(m.info().n_voxels) == 0
        a, b = capi.nn_search(m, queries, I12, 1.0), capi.nn_search(twin, queries, I12, 1.0)
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (name, k)
        # a following insertion with far-voxel removal: freed cap slots are free again, clearance sees only what is left
        m.insert(nxt, T_next, 25.0)
        twin.insert(nxt, T_next, 25.0)
        _same_download(m.download(), twin.download())
        _same_download(m.download_ndt(), twin.download_ndt())
        assert _info(m) == _info(twin), name
        m.close()
        twin.close()
    src_map.close()


def test_erase_points_refuses_a_wrong_count_and_takes_device_flags(capi, lv, ctx):
    import torch
    m = _filled(capi, ctx, "capped")
    d = m.download()
    n = len(d["xyz"])
    for wrong in (n - 1, n + 1, 0):
        with pytest.raises(capi.MolahipError) as e:
            lv.erase_points(m, np.ones(wrong, np.uint8))
        assert e.value.status == 1
    assert lv.lib().mh_map_erase_points(None, None, 0, capi.MEM_HOST) == 1
    assert lv.lib().mh_map_erase_points(m._h, None, n, capi.MEM_HOST) == 1
    assert lv.lib().mh_map_erase_points(m._h, None, n, 9) == 1
    _same_download(m.download(), d)                  # untouched
    assert lv.erased_total(m) == 0
    drop = np.arange(n) % 3 == 0
    flags = torch.from_numpy(drop.astype(np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    lv.erase_points_device(m, flags.data_ptr(), n)
    _same_download(m.download(), _twin(capi, ctx, "capped", d, int(m.info().n_offered), ~drop).download())
    empty = capi.Map(ctx, **MAP_KINDS["capped"])
    lv.erase_points(empty, np.zeros(0, np.uint8))    # nothing stored, nothing to do
    assert int(empty.info().n_points) == 0
    m.close()


# ------------------------------------------------------------------ mh_map_erase_seen_through
@pytest.mark.parametrize("kind", sorted(MAP_KINDS))
def test_erase_seen_through_is_vote_decide_erase(capi, cl, lv, ctx, kind):
    p = _params(32, 128, win_rings=0, win_sectors=1)
    v, views = _store(cl, ctx, p, 700)
    src_map = _filled(capi, ctx, kind)
    d, n_off = src_map.download(), int(src_map.info().n_offered)
    rng = np.random.default_rng(8)
    nv, nT = _nbr(rng, len(views), 24, spread=3.0)
    votes = lv.vote_map(v, src_map, nv, nT)
    assert votes.tobytes() == cr.vote(d["xyz"], views, nv, nT, **p).tobytes()
    seen = set()
    for mt in (1, 2, 3):
        for aw in (0, 1, 2):
            drop = cr.decide(votes, min_through_votes=mt, agree_weight=aw)
            seen.add(int(drop.sum()))
            a, b = _twin(capi, ctx, kind, d, n_off), _twin(capi, ctx, kind, d, n_off)
            lv.erase_seen_through(a, v, nv, nT, mt, aw)
            lv.erase_points(b, drop)
            _same_download(a.download(), b.download())
            _same_download(a.download_ndt(), b.download_ndt())
            assert _info(a) == _info(b)
            assert lv.erased_total(a) == int(drop.sum()) == lv.erased_total(b)
            # a second, queued call on what is left: the totals add up
            left = a.download()["xyz"]
            again = cr.decide(cr.vote(left, views, nv[:5], nT[:5], **p), min_through_votes=1, agree_weight=aw)
            lv.erase_seen_through(a, v, nv[:5], nT[:5], 1, aw)
            lv.erase_seen_through(a, v, [], np.zeros((0, 12)), 1, 0)   # no neighbours: no votes, nothing goes
            assert lv.erased_total(a) == int(drop.sum()) + int(again.sum())
            assert int(a.info().n_points) == len(d["xyz"]) - lv.erased_total(a)
            a.close()
            b.close()
    assert len(seen) >= 3 and max(seen) > 0   # (the thresholds decided differently)
    v.close()
    src_map.close()


def test_memory_returns_after_destroy(capi, cl, lv):
    probe = capi.Context(0)
    p = _params(32, 128)

    def one_run():
        c = capi.Context(0)
        v = cl.Views(c, cl.clean_params(**p))
        m = _filled(capi, c, "ndt")
        for k in range(3):
            lv.put_scan(v, k, capi.Scan(c, _shell(p, 20000, 8.0 + 10 * k, 12.0 + 10 * k, k)))
        lv.erase_seen_through(m, v, [0, 1, 2], [I12] * 3, 1, 1)
        lv.erase_points(m, np.arange(int(m.info().n_points)) % 2)
        assert lv.erased_total(m) > 0
        c.close()
        gc.collect()
        return probe.memory_info()[0]

    first = one_run()
    assert one_run() == first == one_run()
    probe.close()


def test_a_pending_verdict_stays_pending_across_an_erasing(capi, cl, lv, ctx):
    """an insertion that left out-of-range points out is reported by the NEXT insertion (molahip.h), once, whether the erasing in
    between was queued behind the insertion's counts (erase_seen_through) or had taken them in (erase_points)"""
    import warnings
    p = _params(32, 128)
    v = cl.Views(ctx, cl.clean_params(**p)).add_frames([_shell(p, 20000, 30.0, 40.0, 1)])
    wild = np.concatenate([_dense(500, 61), np.array([[2.0e6, 0, 0]], F)])
    for queued in (True, False):
        m = capi.Map(ctx, **MAP_KINDS["capped"])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m.insert(capi.Scan(ctx, _dense(800, 60)), I12)
            m.insert(capi.Scan(ctx, wild), I12)          # inserted; its verdict is deferred
            if queued:
                lv.erase_seen_through(m, v, [0], [I12], 1, 0)
            else:
                lv.erase_points(m, np.arange(int(m.info().n_points)) % 5 == 0)
            lv.erase_seen_through(m, v, [0, 0], [I12, I12], 1, 0)
        with pytest.warns(RuntimeWarning):
            m.insert(capi.Scan(ctx, _dense(300, 62)), I12)
        with warnings.catch_warnings():
            warnings.simplefilter("error")               # reported once
            lv.erase_seen_through(m, v, [0], [I12], 3, 2)
            m.insert(capi.Scan(ctx, _dense(300, 63)), I12)
            assert int(m.info().deferred_status) == 0
        assert lv.erased_total(m) > 0
        m.close()
    v.close()
