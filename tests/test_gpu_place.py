"""The place-recognition entry points (mh_place_describe, mh_place_db_*, mh_place_search) against tests/place_ref.py, the numpy
restatement of the header's rule.  Every comparison is exact: descriptors byte for byte, matches entry by entry; there are no
tolerances.  tests/test_place_cpu.py checks the restatement itself."""
import ctypes as C

import numpy as np
import pytest

import place_ref as pr
from mola_lidar_odometry_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, UNSUPPORTED = 1, 6
SHAPES = [(20, 64), (1, 8), (32, 128), (5, 24)]   # (5, 24): sectors that are no power of two, two descriptors per workgroup and idle lanes


def _params(R, S):
    return dict(pr.DEFAULT, n_rings=R, n_sectors=S)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch


@pytest.mark.parametrize("n", [0, 1, 255, 257, 5000])
@pytest.mark.parametrize("R,S", SHAPES)
def test_describe_byte_for_byte(ctx, torch_dev, R, S, n):
    torch = torch_dev
    p = _params(R, S)
    cp = capi.place_params(**p)
    for seed in (1, 2):
        xyz = pr.edge_cloud(n, 100 * seed + n, **p)
        ref = pr.describe(xyz, **p)
        s = capi.Scan(ctx, xyz)
        got = capi.place_describe(s, cp)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
        d = torch.full((R * S,), 7, dtype=torch.uint8, device="cuda")  # the output in device memory
        capi.place_describe_device(s, cp, d.data_ptr())
        assert np.array_equal(d.cpu().numpy().reshape(R, S), ref)
        s.close()
        if n >= 255:
            assert ref.any()


@pytest.mark.parametrize("R,S", SHAPES)
def test_a_quarter_turn_shifts_by_a_quarter_of_the_columns(ctx, R, S):
    p = _params(R, S)
    cp = capi.place_params(**p)
    xyz = pr.edge_cloud(5000, 7, **p)
    s, st = capi.Scan(ctx, xyz), capi.Scan(ctx, pr.quarter_turn(xyz))
    d, dt = capi.place_describe(s, cp), capi.place_describe(st, cp)
    assert np.array_equal(np.roll(d, S // 4, axis=1), dt)
    assert np.array_equal(dt, pr.describe(pr.quarter_turn(xyz), **p))
    assert (d > 0).any(axis=0).all() and (d > 0).any(axis=1).all()  # every sector and every ring is reached
    s.close()
    st.close()


def _frames(rng, sizes, p):
    return [pr.edge_cloud(int(n), int(rng.integers(1 << 30)), **p) for n in sizes]


def _queries(rng, R, S, descs):
    q = [rng.integers(0, 256, (R, S), dtype=np.uint8), np.zeros((R, S), np.uint8)]
    q += [np.roll(d, 3, axis=1) for d in descs[:2]]
    return q


@pytest.mark.parametrize("n_frames", [1, 3, 40])
@pytest.mark.parametrize("R,S", SHAPES)
def test_add_frames_equals_the_loop_of_describe_and_add(ctx, torch_dev, R, S, n_frames):
    torch = torch_dev
    p = _params(R, S)
    cp = capi.place_params(**p)
    rng = np.random.default_rng(R * 1000 + n_frames)
    sizes = rng.integers(0, 3001, n_frames)
    if n_frames >= 3:
        sizes[1] = 0
    if n_frames == 40:
        sizes[[0, 17, 18, 39]] = 0
        sizes[5] = 1
    frames = _frames(rng, sizes, p)
    loop, host, dev, split = (capi.PlaceDB(ctx, cp) for _ in range(4))
    descs = []
    for f in frames:
        s = capi.Scan(ctx, f)
        descs.append(capi.place_describe(s, cp))
        loop.add(descs[-1])
        s.close()
    assert all(np.array_equal(d, pr.describe(f, **p)) for d, f in zip(descs, frames))
    host.add_frames(frames)
    keep = [[torch.from_numpy(np.ascontiguousarray(f[:, a])).cuda() for a in range(3)] for f in frames]
    dev.add_frames_device([(x.data_ptr() if len(x) else None, y.data_ptr() if len(y) else None, z.data_ptr() if len(z) else None,
                            len(x)) for x, y, z in keep])
    cut = n_frames // 2
    split.add_frames(frames[:cut])  # (an empty group the first time with one frame)
    split.add_frames(frames[cut:])
    for db in (loop, host, dev, split):
        assert len(db) == n_frames
    ref_stack = np.stack(descs)
    for q in _queries(rng, R, S, descs):
        want = loop.search(q)
        rs, rd = pr.search(ref_stack, q)
        assert np.array_equal(want["shift"], rs) and np.array_equal(want["dist"], rd)
        for db in (host, dev, split):
            got = db.search(q)
            assert np.array_equal(got, want)
    for db in (loop, host, dev, split):
        db.close()


@pytest.mark.parametrize("K", [1, 3, 257])
@pytest.mark.parametrize("R,S", SHAPES)
def test_search_every_entry(ctx, torch_dev, R, S, K):
    torch = torch_dev
    cp = capi.place_params(**_params(R, S))
    rng = np.random.default_rng(K * 131 + S)
    stored = rng.integers(0, 256, (K, R, S), dtype=np.uint8)
    stored[0] = 0  # an all-empty descriptor
    if K >= 3:
        stored[2] = stored[1]  # two identical ones
    j = K - 1
    queries = [rng.integers(0, 256, (R, S), dtype=np.uint8),
               np.roll(stored[j], 5 % S, axis=1),                  # a column roll of frame j: dist 0 at that shift
               np.roll(stored[j], S - 1, axis=1),
               np.full((R, S), 200, np.uint8),                     # a constant query: every shift ties, the answer is shift 0
               np.zeros((R, S), np.uint8)]
    sparse = rng.integers(0, 256, (R, S), dtype=np.uint8) * (rng.random((R, S)) < 0.3)
    queries.append(sparse.astype(np.uint8))
    db = capi.PlaceDB(ctx, cp).add(stored[:K // 2]).add(stored[K // 2:])
    assert len(db) == K
    for qi, q in enumerate(queries):
        got = db.search(q)
        rs, rd = pr.search(stored, q)
        assert np.array_equal(got["shift"], rs) and np.array_equal(got["dist"], rd), qi
        if qi == 1 and K > 1:
            assert got["dist"][j] == 0 and got["shift"][j] == 5 % S
        if qi == 3:
            assert not got["shift"].any()
    # query and matches in device memory
    q = torch.from_numpy(queries[0].reshape(-1)).cuda()
    out = torch.zeros((K, 2), dtype=torch.int32, device="cuda")
    db.search_device(q.data_ptr(), out.data_ptr())
    got = out.cpu().numpy().astype(np.uint32)
    rs, rd = pr.search(stored, queries[0])
    assert np.array_equal(got[:, 0], rs) and np.array_equal(got[:, 1], rd)
    # descriptors appended from device memory
    db2 = capi.PlaceDB(ctx, cp)
    dd = torch.from_numpy(stored.reshape(-1)).cuda()
    db2.add_device(dd.data_ptr(), K)
    assert np.array_equal(db2.search(queries[0]), db.search(queries[0]))
    db.close()
    db2.close()


def test_dist_at_shift_zero_is_the_plain_l1_distance(ctx):
    """two nearly equal clouds: the restatement puts the best shift at 0, and there the distance is the plain L1 distance of the
    two mh_place_describe outputs"""
    p = _params(20, 64)
    cp = capi.place_params(**p)
    a = pr.edge_cloud(3000, 11, **p)
    b = (a + np.random.default_rng(3).normal(0, 0.02, a.shape)).astype(F)
    sa, sb = capi.Scan(ctx, a), capi.Scan(ctx, b)
    da, db_ = capi.place_describe(sa, cp), capi.place_describe(sb, cp)
    l1 = int(np.abs(da.astype(np.int64) - db_.astype(np.int64)).sum())
    D = pr.distances(db_[None], da)
    assert l1 > 0 and D[0, 0] == l1 and int(np.argmin(D[0])) == 0
    db = capi.PlaceDB(ctx, cp).add(db_).add(da)
    got = db.search(da)
    assert got["shift"][0] == 0 and got["dist"][0] == l1
    assert got["shift"][1] == 0 and got["dist"][1] == 0  # the descriptor against itself
    for h in (sa, sb, db):
        h.close()


def test_refusals_leave_the_database_untouched(ctx):
    L = capi.lib()
    p = _params(1, 8)
    cp = capi.place_params(**p)
    xyz = pr.edge_cloud(300, 5, **p)
    s = capi.Scan(ctx, xyz)
    db = capi.PlaceDB(ctx, cp).add(pr.describe(xyz, **p))
    buf = np.zeros(8, np.uint8)
    out = np.zeros(4, capi.PLACE_MATCH_DTYPE)
    fr = (capi.MapFrame * 1)()
    x, y, z = capi._soa(xyz)
    fr[0].x, fr[0].y, fr[0].z, fr[0].n = capi._vp(x), capi._vp(y), capi._vp(z), len(x)
    nullfr = (capi.MapFrame * 1)()
    nullfr[0].n = 5
    h = C.c_void_p()
    n64 = C.c_uint64()
    vp = capi._vp
    bad_params = [dict(n_rings=0), dict(n_rings=33), dict(n_sectors=0), dict(n_sectors=12), dict(n_sectors=136),
                  dict(min_range=-1.0), dict(min_range=80.0), dict(max_range=float("inf")), dict(max_range=float("nan")),
                  dict(z_min=27.0), dict(z_min=float("nan")), dict(z_max=float("inf")), dict(max_range=1e30)]
    calls = [
        (INVALID, lambda: L.mh_place_describe(None, C.byref(cp), vp(buf), capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_describe(s._h, None, vp(buf), capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_describe(s._h, C.byref(cp), None, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_describe(s._h, C.byref(cp), vp(buf), 3)),
        (INVALID, lambda: L.mh_place_describe(s._h, C.byref(cp), vp(buf), -1)),
        (INVALID, lambda: L.mh_place_db_create(None, C.byref(cp), C.byref(h))),
        (INVALID, lambda: L.mh_place_db_create(ctx._h, None, C.byref(h))),
        (INVALID, lambda: L.mh_place_db_create(ctx._h, C.byref(cp), None)),
        (INVALID, lambda: L.mh_place_db_size(None, C.byref(n64))),
        (INVALID, lambda: L.mh_place_db_size(db._h, None)),
        (INVALID, lambda: L.mh_place_db_add(None, vp(buf), 1, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_db_add(db._h, None, 1, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_db_add(db._h, vp(buf), 1, 7)),
        (INVALID, lambda: L.mh_place_db_add_frames(None, fr, 1, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_db_add_frames(db._h, None, 1, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_db_add_frames(db._h, fr, 1, 9)),
        (INVALID, lambda: L.mh_place_db_add_frames(db._h, nullfr, 1, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_search(None, vp(buf), capi.MEM_HOST, vp(out), capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_search(db._h, None, capi.MEM_HOST, vp(out), capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_search(db._h, vp(buf), capi.MEM_HOST, None, capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_search(db._h, vp(buf), 5, vp(out), capi.MEM_HOST)),
        (INVALID, lambda: L.mh_place_search(db._h, vp(buf), capi.MEM_HOST, vp(out), 5)),
    ]
    for bad in bad_params:
        bp = capi.place_params(**dict(p, **bad))
        calls.append((INVALID, lambda bp=bp: L.mh_place_describe(s._h, C.byref(bp), vp(buf), capi.MEM_HOST)))
        calls.append((INVALID, lambda bp=bp: L.mh_place_db_create(ctx._h, C.byref(bp), C.byref(h))))
    # more than MH_PLACE_MAX_DESCRIPTORS: in one call, and by the sum with what is stored
    big = np.zeros((capi.PLACE_MAX_DESCRIPTORS + 1, 8), np.uint8)
    manyfr = (capi.MapFrame * (capi.PLACE_MAX_DESCRIPTORS + 1))()
    calls.append((UNSUPPORTED, lambda: L.mh_place_db_add(db._h, vp(big), len(big), capi.MEM_HOST)))
    calls.append((UNSUPPORTED, lambda: L.mh_place_db_add(db._h, vp(big), capi.PLACE_MAX_DESCRIPTORS, capi.MEM_HOST)))
    calls.append((UNSUPPORTED, lambda: L.mh_place_db_add_frames(db._h, manyfr, len(manyfr), capi.MEM_HOST)))
    calls.append((UNSUPPORTED, lambda: L.mh_place_db_add_frames(db._h, manyfr, capi.PLACE_MAX_DESCRIPTORS, capi.MEM_HOST)))
    before = db.search(pr.describe(xyz, **p)).copy()
    for i, (want, call) in enumerate(calls):
        assert int(call()) == want, i
        assert len(db) == 1, i
        assert L.mh_last_error_string()
    # after the refusals good calls succeed and the content is what it was
    assert np.array_equal(capi.place_describe(s, cp), pr.describe(xyz, **p))
    assert np.array_equal(db.search(pr.describe(xyz, **p)), before) and before["dist"][0] == 0
    db.add_frames([xyz])
    assert len(db) == 2 and not db.search(pr.describe(xyz, **p))["dist"].any()
    # the database filled to the limit takes nothing more and still answers
    db.add(big[:capi.PLACE_MAX_DESCRIPTORS - 2])
    assert len(db) == capi.PLACE_MAX_DESCRIPTORS
    assert int(L.mh_place_db_add(db._h, vp(buf), 1, capi.MEM_HOST)) == UNSUPPORTED
    assert int(L.mh_place_db_add_frames(db._h, fr, 1, capi.MEM_HOST)) == UNSUPPORTED
    assert len(db) == capi.PLACE_MAX_DESCRIPTORS
    got = db.search(pr.describe(xyz, **p))
    assert got["dist"][0] == 0 and got["dist"][1] == 0 and len(got) == capi.PLACE_MAX_DESCRIPTORS
    s.close()
    db.close()


def test_trivial_cases(ctx):
    p = _params(20, 64)
    cp = capi.place_params(**p)
    empty = capi.Scan(ctx, np.zeros((0, 3), F))
    assert not capi.place_describe(empty, cp).any()  # an empty scan: all zeros
    db = capi.PlaceDB(ctx, cp)
    out = np.full(3, 77, np.uint32)
    q = np.zeros((20, 64), np.uint8)
    assert int(capi.lib().mh_place_search(db._h, capi._vp(q), capi.MEM_HOST, capi._vp(out), capi.MEM_HOST)) == 0
    assert (out == 77).all()  # a search of an empty database writes nothing
    db.add(np.zeros((0, 20, 64), np.uint8))  # n_desc == 0 changes nothing
    db.add_frames([])
    assert len(db) == 0
    db.add_frames([np.zeros((0, 3), F)])  # an empty frame: an all-zero descriptor
    assert len(db) == 1
    got = db.search(q)
    assert got["dist"][0] == 0 and got["shift"][0] == 0
    empty.close()
    db.close()
