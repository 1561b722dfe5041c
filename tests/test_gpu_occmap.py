"""The occupancy voxel map (mh_occmap, the mrpt::maps::CVoxelMap stand-in) through the C ABI against the numpy restatement
tests/occmap_ref.py: bit-exact on cell indices, log-odds, the occupied list, the info counters and the inner search map."""
import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

import occmap_ref as R

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def pose(x=0.0, y=0.0, z=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, z], np.float64)


def make(ctx, **kw):
    """The device map and its restatement with the same parameters."""
    occ = capi.OccMap(ctx, **kw)
    kw.pop("search_voxel_size", None)
    kw.pop("max_keys_per_pass", None)
    if "index_mode" in kw:
        kw["trunc"] = kw.pop("index_mode") == capi.INDEX_TRUNC
    return occ, R.OccMapRef(**kw)


def insert_both(ctx, occ, ref, xyz, T, far=0.0):
    s = capi.Scan(ctx, np.asarray(xyz, F).reshape(-1, 3))
    occ.insert(s, T, far)
    s.close()
    ref.insert(xyz, T, far)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(occ, ref, counters=True):
    """Cells, log-odds, info counters, and the inner map's content against the restatement, bit for bit."""
    keys, lo = occ.download()
    rk, rl = ref.download()
    assert keys.shape == rk.shape and np.array_equal(keys, rk)
    assert np.array_equal(lo, rl)
    info = occ.info()
    cen = ref.centres()
    assert (info.l_hit, info.l_miss, info.l_min, info.l_max, info.l_occ) == (ref.l_hit, ref.l_miss, ref.l_min, ref.l_max, ref.l_occ)
    assert info.n_cells == len(rk) and info.n_occupied == len(cen)
    if counters:
        assert info.n_left_out == ref.n_left_out and info.n_keys == ref.n_keys
    d = occ.search_map(0.0).download()
    assert len(d["src_idx"]) == len(cen)
    order = np.argsort(d["src_idx"], kind="stable")
    assert np.array_equal(d["src_idx"][order], np.arange(len(cen), dtype=np.uint32))  # global index = rank in key order
    assert np.array_equal(bits(d["xyz"][order]), bits(cen))
    return keys, lo


def ball(n, radius, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p *= (radius * rng.random(n) ** (1 / 3) / np.linalg.norm(p, axis=1))[:, None]
    return p.astype(F)


@pytest.mark.parametrize("rule", [capi.OCC_COUNTED, capi.OCC_ONCE])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_point_counts(ctx, n, rule):
    occ, ref = make(ctx, resolution=0.25, update_rule=rule)
    pts = ball(n, 5.0, n)
    insert_both(ctx, occ, ref, pts, pose(0.3, -0.2, 0.1, 0.4))
    check(occ, ref)
    insert_both(ctx, occ, ref, pts, pose(1.1, 0.7, -0.4, -1.0))  # the second one meets a non-empty store
    check(occ, ref)
    assert occ.info().n_passes == 1
    occ.close()


def hand_built():
    r = 0.1
    c = lambda i, j, k: [(i + 0.5) * r, (j + 0.5) * r, (k + 0.5) * r]  # centre of a cell
    pts = [[0.02, 0.03, 0.01], c(1, 0, 0), c(0, -1, 0)]   # in the origin's cell; adjacent cells
    pts += [c(1, 0, 0)] * 150                             # 1-cell rays ...
    pts += [c(700, 3, -2)]                                # ... a 700-cell ray between them ...
    pts += [c(0, 1, 0), c(0, 0, -1)] * 150                # ... and more: its items span several workgroups
    pts += [c(5, 5, 5), c(-7, -7, -7), c(12, -12, 0), c(0, 9, 9)]  # exact diagonals
    pts += [[-3.21, -0.77, -1.5], [-0.001, -0.001, -0.001]]        # negative coordinates
    pts += [[2.31 + 0.001 * i, 1.12, 0.33] for i in range(40)]      # 40 points in one cell
    pts += [c(0, -3, 0), c(0, -7, 0), c(7, 7, 0), c(3, 3, 0)]      # rays through other rays' end cells
    pts += [[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]]
    pts += [[90.0, 1.0, 0.0]]                                      # beyond max_range = 80 where that is set
    pts += [[1.2e5, 0.0, 0.0]]                                     # index beyond the key range (1.2e6 cells)
    pts += [c(-4, 2, 1)]
    return np.array(pts, F)


@pytest.mark.parametrize("cfg", [dict(), dict(max_range=80.0), dict(decimation=3), dict(ray_trace_free_space=False),
                                 dict(update_rule=capi.OCC_ONCE), dict(index_mode=capi.INDEX_TRUNC)],
                         ids=["default", "max_range", "decimation3", "no_ray_trace", "once", "trunc"])
def test_hand_built_rays(ctx, cfg):
    occ, ref = make(ctx, resolution=0.1, **cfg)
    pts = hand_built()
    T = pose()  # (the origin's cell is (0, 0, 0); the points land on the cell centres they were built from)
    insert_both(ctx, occ, ref, pts, T)
    keys, lo = check(occ, ref)
    cells = {tuple(k): int(l) for k, l in zip(keys.tolist(), lo.tolist())}
    info = occ.info()
    if not cfg:
        assert info.n_left_out == 1                   # the point at 1.2e5 m, and everything else is in
        assert cells[(23, 11, 3)] == 47               # 40 hits: clamped at l_max
        assert cells[(0, 0, 0)] == 14 and cells[(700, 3, -2)] == 14 and cells[(900, 10, 0)] == 14
        assert cells[(0, -3, 0)] == 0 and cells[(3, 3, 0)] == 0  # one hit, one miss from the ray that goes on behind it
        assert cells[(0, -5, 0)] == -14 and cells[(1, 1, 1)] == -14  # in-between cells of one ray each
    if cfg.get("update_rule") == capi.OCC_ONCE:
        assert cells[(0, -3, 0)] == 14 and cells[(23, 11, 3)] == 14  # a hit wins, and counts once
    if cfg.get("max_range"):
        assert (900, 10, 0) not in cells and info.n_left_out == 0  # (the far-out point falls to the range test first)
    if cfg.get("ray_trace_free_space") is False:
        assert min(cells.values()) >= 14 and info.n_keys == len(pts) - 3 - 1  # hits only: the finite points inside the range
    insert_both(ctx, occ, ref, pts, pose(-0.31, 0.22, 0.05, 2.0))
    check(occ, ref)
    occ.close()


def test_pass_size_does_not_change_the_result(ctx):
    pts = ball(1000, 2.0, 7)
    got = []
    for per_pass in (0, 256, 1):
        occ, ref = make(ctx, resolution=0.5, max_keys_per_pass=per_pass)
        insert_both(ctx, occ, ref, pts, pose(0.1, 0.2, 0.3, 0.5))
        insert_both(ctx, occ, ref, pts[::3], pose(0.6, -0.4, 0.1, 0.1))
        check(occ, ref)
        info = occ.info()
        got.append((occ.download(), info.n_passes, info.n_keys))
        occ.close()
    (k0, l0), p0, nk0 = got[0]
    assert p0 == 1
    for (k, l), p, nk in got[1:]:
        assert p > 1 and nk == nk0
        assert np.array_equal(k, k0) and np.array_equal(l, l0)
    assert got[2][1] == got[2][2]  # one key per pass


def wall(x, n=41):
    return np.stack([np.full(n, x), np.linspace(-1.0, 1.0, n), np.zeros(n)], 1).astype(F)


@pytest.mark.parametrize("rule", [capi.OCC_COUNTED, capi.OCC_ONCE])
def test_saturation_and_erosion(ctx, rule):
    occ, ref = make(ctx, resolution=0.1, update_rule=rule)
    for _ in range(6):
        insert_both(ctx, occ, ref, wall(2.0), pose(0.03, 0.02, 0.0))
        check(occ, ref)
    keys, lo = occ.download()
    hit = keys[:, 0] == 20
    assert hit.any() and (lo[hit] == ref.l_max).all()          # six inserts: every wall cell sits at the upper clamp
    n_occ0 = occ.info().n_occupied
    assert n_occ0 == int(hit.sum())
    for _ in range(10):  # a farther wall seen from a moved origin: the rays cross the first wall's cells
        insert_both(ctx, occ, ref, wall(4.0), pose(-0.5, 0.04, 0.0))
        check(occ, ref)
    keys, lo = occ.download()
    old = lo[keys[:, 0] == 20]
    assert (old < ref.l_occ).any() and old.min() == ref.l_min  # eroded below the threshold, down to the lower clamp
    xyz = occ.search_map(0.0).download()["xyz"]  # ... and those cells have left the search map
    assert int((np.abs(xyz[:, 0] - 2.05) < 1e-3).sum()) == int((old >= ref.l_occ).sum()) < n_occ0
    occ.close()


@pytest.mark.parametrize("metric", [capi.FAR_CHEBYSHEV, capi.FAR_L1, capi.FAR_L2])
def test_far_removal_and_recreation(ctx, metric):
    occ, ref = make(ctx, resolution=0.2, far_voxel_metric=metric)
    pts = ball(300, 5.0, 3)
    insert_both(ctx, occ, ref, pts, pose(0.1, 0.1, 0.1))
    n0 = occ.info().n_cells
    before = dict(ref.cells)
    insert_both(ctx, occ, ref, pts[:5] * F(0.1), pose(3.0, 0.1, 0.1), far=2.0)
    check(occ, ref)
    assert 0 < occ.info().n_cells < n0
    cell = sorted(c for c, l in before.items() if l != 0 and c not in ref.cells)[0]  # a cell the removal erased
    centre = (np.array(cell, np.float64) + 0.5) * 0.2
    insert_both(ctx, occ, ref, np.zeros((1, 3), F), pose(*centre), far=0.0)  # one hit, from inside the cell itself
    keys, lo = check(occ, ref)
    at = np.flatnonzero((keys == np.array(cell)).all(axis=1))
    assert len(at) == 1 and lo[at[0]] == ref.l_hit  # re-created at log-odds 0, then one hit
    occ.close()


def run_sequence(ctx):
    occ = capi.OccMap(ctx, resolution=0.2)
    out = []
    for i in range(4):
        s = capi.Scan(ctx, ball(500, 4.0, 10 + i))
        occ.insert(s, pose(0.4 * i, -0.2 * i, 0.0, 0.3 * i), 6.0 if i == 3 else 0.0)
        s.close()
        out.append(occ.download() + (occ.search_map(0.0).download()["xyz"],))
    occ.close()
    return out


def test_repeatability(ctx):
    a, b = run_sequence(ctx), run_sequence(ctx)
    for x, y in zip(a, b):
        assert all(np.array_equal(u.view(np.uint32) if u.dtype == F else u, v.view(np.uint32) if v.dtype == F else v)
                   for u, v in zip(x, y))


def test_clear_behaves_as_new(ctx):
    occ, ref = make(ctx, resolution=0.2)
    insert_both(ctx, occ, ref, ball(400, 4.0, 1), pose(0.1, 0.2, 0.3))
    occ.search_map(2.5)
    assert occ.info().search_voxel_size == 4.0
    occ.clear()
    ref.clear()
    info = occ.info()
    assert info.n_cells == 0 and info.n_occupied == 0 and info.search_voxel_size == 1.0
    assert len(occ.search_map(0.0).download()["src_idx"]) == 0
    check(occ, ref, counters=False)
    insert_both(ctx, occ, ref, ball(400, 4.0, 2), pose(-0.1, 0.0, 0.3))
    check(occ, ref)
    occ.close()


@pytest.fixture(scope="module")
def room(ctx):
    """A map of a box-shaped room's walls and its restatement (shared, left unchanged by the tests that use it)."""
    occ, ref = make(ctx, resolution=0.1)
    rng = np.random.default_rng(5)
    n = 1500
    u, v = rng.uniform(-3, 3, n), rng.uniform(-1, 1, n)
    side = rng.integers(0, 4, n)
    pts = np.where((side == 0)[:, None], np.stack([np.full(n, 3.0), u, v], 1),
                   np.where((side == 1)[:, None], np.stack([np.full(n, -3.0), u, v], 1),
                            np.where((side == 2)[:, None], np.stack([u, np.full(n, 3.0), v], 1),
                                     np.stack([u, np.full(n, -3.0), v], 1)))).astype(F)
    for _ in range(2):
        insert_both(ctx, occ, ref, pts, pose(0.02, 0.03, 0.01))
    yield occ, ref, pts
    occ.close()


def expected_k2(cen, q, thr):
    idx, d2, full = R.nn_k_bruteforce(cen, q, 2)
    thr2 = F(np.float64(thr) * np.float64(thr))
    li, gi, dd = [], [], []
    for i in range(len(q)):
        for j in range(idx.shape[1]):
            if not d2[i, j] < thr2:
                break
            li.append(i); gi.append(idx[i, j]); dd.append(d2[i, j])
    return np.array(li, np.uint32), np.array(gi, np.uint32), np.array(dd, F), full


@pytest.mark.parametrize("radius,V", [(0.0, 1.0), (2.5, 4.0)], ids=["within_V", "growth"])
def test_search_equals_brute_force(ctx, room, radius, V):
    occ, ref, pts = room
    if radius:  # growth changes the map's search voxel for good: on a device map of its own, against the shared restatement
        occ = capi.OccMap(ctx, resolution=0.1)
        s = capi.Scan(ctx, pts)
        for _ in range(2):
            occ.insert(s, pose(0.02, 0.03, 0.01))
        s.close()
        assert occ.info().search_voxel_size == 1.0
    cen = ref.centres()
    thr = 1.0 if radius == 0.0 else 2.5
    rng = np.random.default_rng(11)
    q = rng.uniform(-3.3, 3.3, (400, 3)).astype(F) * np.array([1, 1, 0.3], F)
    full = R.nn_k_bruteforce(cen, q, 2)[2]
    ok = (full[:, 0] < full[:, 1]) & (full[:, 1] < full[:, 2])  # the reference alone shows the gaps: no tie decides
    q = q[ok]
    assert len(q) > 300
    li, gi, dd, full = expected_k2(cen, q, thr)
    assert ((full[:, 1] - full[:, 0]) > 0).all() and ((full[:, 2] - full[:, 1]) > 0).all()
    m = occ.search_map(radius)
    assert occ.info().search_voxel_size == V
    s = capi.Scan(ctx, q)
    got = capi.nn_search_k(m, s, pose(), thr, 2)
    s.close()
    assert len(li) > len(q) // 2  # (most queries do find their two)
    if radius:
        assert (np.sqrt(dd.astype(np.float64)) > 1.0).any()  # pairs beyond the first V are among them
    assert np.array_equal(got["local_idx"], li) and np.array_equal(got["global_idx"], gi)
    assert np.array_equal(bits(got["d2"]), bits(dd))
    assert np.array_equal(bits(got["global_xyz"]), bits(cen[gi]))
    if radius:
        occ.close()


def test_alignment_equals_a_plain_map_of_the_centres(ctx, room):
    occ, ref, pts = room
    cen = ref.centres()
    m_occ = occ.search_map(1.0)
    V = occ.info().search_voxel_size
    plain = capi.Map(ctx, V, 0).build(cen)
    c, s_ = np.cos(0.03), np.sin(0.03)
    Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]])
    local = ((pts[:700].astype(np.float64) - np.array([0.08, -0.05, 0.02])) @ Rz).astype(F)
    scan = capi.Scan(ctx, local)
    p = capi.ICPParams(max_iterations=40, threshold=0.8, kernel_param=0.3)
    out = []
    for m in (m_occ, plain):
        out.append(capi.icp_align_layers([dict(map=m, scan=scan, threshold=0.8)], pose(), p, want_pairs=True, pairings_per_point=2))
    a, b = out
    assert a["n_iterations"] == b["n_iterations"] and a["n_iterations"] > 1
    assert a["n_final_pairs"] == b["n_final_pairs"] and a["n_final_pairs"] > 700
    assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64))
    for k in ("local_idx", "global_idx"):
        assert np.array_equal(a["pairs"][0][k], b["pairs"][0][k])
    assert np.array_equal(bits(a["pairs"][0]["d2"]), bits(b["pairs"][0]["d2"]))
    scan.close()
    plain.close()


def test_a_scan_of_another_context_is_refused(ctx):
    other = capi.Context(0)
    occ = capi.OccMap(ctx)
    s = capi.Scan(other, np.zeros((3, 3), F))
    with pytest.raises(capi.MolahipError) as e:
        occ.insert(s, pose())
    assert e.value.status == 1 and "different contexts" in str(e.value)
    assert occ.info().n_cells == 0
    occ.close()
    other.close()
