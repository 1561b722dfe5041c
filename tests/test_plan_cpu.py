"""The restatement of include/molahip_plan.h (tests/plan_ref.py) held to a second method, and the host rules of
mola_lidar_odometry_hip/RoutePlan.h through pybind: the price table, the cell rule, the route: block and its refusals, the summary,
the files.  No device is asked for."""
import math

import numpy as np
import pytest

import nav_ref as NR
import plan_cases as pc
import plan_ref as R

INF = np.int64(1) << 62


def relaxed_field(cost, goals_xy, price, below=253):
    """the field by repeated relaxation of the whole plane against its eight shifted copies, to a fixed point (Bellman-Ford on
    arrays): shaped nothing like the heap of plan_ref.field"""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    ok = cost < below
    p = np.where(ok, np.asarray(price, np.int64)[np.minimum(cost, below - 1)], 0)
    okp = np.zeros((ny + 2, nx + 2), bool)
    okp[1:-1, 1:-1] = ok
    pp = np.zeros((ny + 2, nx + 2), np.int64)
    pp[1:-1, 1:-1] = p
    f = np.full((ny + 2, nx + 2), INF, np.int64)
    for x, y in np.asarray(goals_xy, np.int64).reshape(-1, 2):
        if 0 <= x < nx and 0 <= y < ny and ok[y, x]:
            f[y + 1, x + 1] = 0
    inner = (slice(1, -1), slice(1, -1))

    def shifted(a, dx, dy):
        return a[1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]

    while True:
        best = f[inner].copy()
        for dx, dy, L in R.STEPS:
            allowed = ok & shifted(okp, dx, dy)
            if dx and dy:
                allowed &= shifted(okp, dx, 0) & shifted(okp, 0, dy)
            cand = shifted(f, dx, dy) + L * (p + shifted(pp, dx, dy))
            best = np.where(allowed & (shifted(f, dx, dy) < INF) & (cand < best), cand, best)
        if (best == f[inner]).all():
            break
        f[inner] = best
    out = f[inner]
    return np.where(out >= INF, R.UNREACHED, out).astype(np.uint32)


@pytest.mark.parametrize("shape", [(1, 1), (70, 1), (1, 70), (33, 9), (70, 40)])
def test_the_restatement_equals_whole_plane_relaxation(shape):
    nx, ny = shape
    for k, lethal in enumerate((0.25, 0.02)):
        cost = pc.random_cost(nx, ny, 7 * nx + ny + k, lethal)
        for price in (pc.stepped(), pc.flat(), pc.by_cost()):
            for goals in pc.goal_lists(cost, k):
                f, info = R.field(cost, goals, price)
                assert np.array_equal(f, relaxed_field(cost, goals, price)), (shape, lethal, len(goals))
                finite = f != R.UNREACHED
                assert info["n_reached"] == finite.sum() and info["max_field"] == (f[finite].max() if finite.any() else 0)


def test_special_planes_in_the_restatement():
    f, _ = R.field(pc.diagonal_touch(12), [[2, 2]], pc.flat())
    assert (f[1:6, 1:6] != R.UNREACHED).all() and (f[6:, 6:] == R.UNREACHED).all()        # touching at a corner does not join
    f, _ = R.field(pc.beside_diagonal(), [[2, 2]], pc.flat())
    assert f[1, 1] == 20 and f[3, 3] == 14 and f[2, 1] == 10                               # 5 + 5 steps of price 1 + 1, not 7
    assert np.array_equal(f, relaxed_field(pc.beside_diagonal(), [[2, 2]], pc.flat()))
    b = pc.serpentine(21)
    f, info = R.field(b, [[0, 0]], pc.flat())
    assert ((f != R.UNREACHED) == (b == 0)).all() and np.array_equal(f, relaxed_field(b, [[0, 0]], pc.flat()))
    assert info["max_field"] == int(f[20, 20])                                             # the far end of the last row, entered at column 0
    # the price decides the route
    b = pc.two_corridors(9)
    for price, row in ((pc.by_cost(), 4), (pc.flat(), 0)):
        f, _ = R.field(b, [[8, 0]], price)
        (route,), (n,) = R.trace(b, f, [[0, 0]], price)
        assert n == len(route) and tuple(route[-1]) == (8, 0) and route[:, 1].max() == row     # over row 4 when cost has a price, along row 0 else


@pytest.mark.parametrize("seed", range(4))
def test_the_finite_cells_are_the_reach_plane(seed):
    """no corner is cut, so 8-connected steps join exactly the cells the 4-connected flood fill joins"""
    rng = np.random.default_rng(seed)
    nx, ny = int(rng.integers(1, 70)), int(rng.integers(1, 40))
    cost = pc.random_cost(nx, ny, 50 + seed, 0.3)
    for below in (253, 100, 1):
        goals = np.concatenate([pc.passable_cells(cost, below)[:3], pc.blocked_cells(cost, below)[:2], pc.outside_cells(nx, ny)[:2]])
        f, info = R.field(cost, goals, pc.stepped(below), below)
        reach, rinfo = NR.reach(cost, goals, below)
        assert np.array_equal(f != R.UNREACHED, reach == 1)
        assert (info["n_reached"], info["n_goals_blocked"], info["n_goals_outside"]) == (rinfo["n_reached"], rinfo["n_seeds_blocked"],
                                                                                         rinfo["n_seeds_outside"])


def test_the_trace_follows_the_field_down():
    cost = pc.random_cost(60, 35, 3, 0.2)
    price = pc.stepped()
    goals = pc.passable_cells(cost)[[5, 400, 900]]
    f, _ = R.field(cost, goals, price)
    starts = np.concatenate([pc.passable_cells(cost)[::37], pc.outside_cells(60, 35)[:2], pc.blocked_cells(cost)[:2]])
    routes, lens = R.trace(cost, f, starts, price)
    for s, r, n in zip(starts.tolist(), routes, lens):
        inside = 0 <= s[0] < 60 and 0 <= s[1] < 35
        if not inside or f[s[1], s[0]] == R.UNREACHED:
            assert n == 0 and len(r) == 0
            continue
        assert n == len(r) and tuple(r[0]) == tuple(s) and f[r[-1, 1], r[-1, 0]] == 0 and (f[r[:-1, 1], r[:-1, 0]] > 0).all()
        for (a, b), (c, d) in zip(r[:-1].tolist(), r[1:].tolist()):
            L = 7 if (a != c and b != d) else 5
            assert int(f[b, a]) - int(f[d, c]) == L * (int(price[cost[b, a]]) + int(price[cost[d, c]]))
        if n > 1:
            cut, cut_len = R.trace(cost, f, [s], price, cap=n - 1)
            assert cut_len == [R.TRUNCATED] and np.array_equal(cut[0], r[:n - 1])
        assert R.trace(cost, f, [s], price, cap=n)[1] == [n]


def test_the_wrap_around_arithmetic():
    assert R.wrap_bound_holds(1 << 24, [18] * 253) and not R.wrap_bound_holds(1 << 24, [19] * 253)         # 4096 x 4096
    assert R.wrap_bound_holds(10 ** 6, [306]) and not R.wrap_bound_holds(10 ** 6, [307])                     # 1000 x 1000
    assert ((1 << 24) - 1) * 14 * 18 == 4227858180 < 0xFFFFFFFF < ((1 << 24) - 1) * 14 * 19 == 4462739190
    for top in (1, 18, 19, 306, 65535):
        n = R.admitted_cells([top])
        assert R.wrap_bound_holds(n, [top]) and not R.wrap_bound_holds(n + 1, [top])


# ---- the host rules through pybind --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def test_the_route_block_and_its_refusals(H):
    d = H.route_options("")
    assert math.isnan(d["start_x"]) and math.isnan(d["goal_y"])
    assert (d["start_keyframe"], d["goal_keyframe"], d["neutral_price"], d["cost_factor"], d["max_route_cells"]) == (0, -1, 4, 0.08, 1048576)
    d = H.route_options("route:\n  start_x: 1.5\n  start_y: -2\n  goal_x: 3\n  goal_y: 4\n  start_keyframe: 3\n  goal_keyframe: 7\n"
                        "  neutral_price: 9\n  cost_factor: 0\n  max_route_cells: 10\n")
    assert (d["start_x"], d["start_y"], d["goal_x"], d["goal_y"], d["start_keyframe"], d["goal_keyframe"], d["neutral_price"], d["cost_factor"],
            d["max_route_cells"]) == (1.5, -2.0, 3.0, 4.0, 3, 7, 9, 0.0, 10)
    for key, value in (("no_such_key", "1"), ("start_x", "nan"), ("goal_x", "inf"), ("start_keyframe", "-2"),
                       ("goal_keyframe", "1.5"), ("neutral_price", "0"), ("neutral_price", "-1"), ("neutral_price", "1.5"), ("cost_factor", "-0.1"),
                       ("cost_factor", "nan"), ("cost_factor", "steep"), ("max_route_cells", "0"), ("max_route_cells", "[1, 2]")):
        with pytest.raises(RuntimeError) as e:
            H.route_options("route:\n  %s: %s\n" % (key, value))
        assert "route:" in str(e.value) and key in str(e.value), (key, str(e.value))
    for key, named in (("start_x", "start_y"), ("start_y", "start_x"), ("goal_x", "goal_y"), ("goal_y", "goal_x")):     # half a point
        with pytest.raises(RuntimeError) as e:
            H.route_options("route:\n  %s: 1\n" % key)
        assert "route:" in str(e.value) and named in str(e.value)


def test_the_price_table(H):
    for np_, cf in ((4, 0.08), (1, 0.0), (7, 1.0), (1, 0.0625), (65535, 0.0), (4, 260.0), (300, 0.3)):
        t = H.route_price_table("route:\n  neutral_price: %d\n  cost_factor: %r\n" % (np_, cf))
        assert t.dtype == np.uint16 and np.array_equal(t, R.price_table(np_, cf))
    assert np.array_equal(H.route_price_table(""), R.price_table()) and len(H.route_price_table("")) == 253
    for text in ("route:\n  neutral_price: 65536\n", "route:\n  cost_factor: 261\n", "route:\n  neutral_price: 65000\n  cost_factor: 3\n"):
        with pytest.raises(RuntimeError) as e:
            H.route_price_table(text)
        assert "route:" in str(e.value) and "65535" in str(e.value)
    # the wrap-around bound: prices up to 18 admit 4096 x 4096 cells, 19 does not, and the message says what 19 admits
    H.route_price_table("route:\n  neutral_price: 18\n  cost_factor: 0\n", 1 << 24)
    with pytest.raises(RuntimeError) as e:
        H.route_price_table("route:\n  neutral_price: 19\n  cost_factor: 0\n", 1 << 24)
    assert "route:" in str(e.value) and str(R.admitted_cells([19])) in str(e.value) and str(1 << 24) in str(e.value)
    H.route_price_table("", R.admitted_cells(R.price_table()))
    with pytest.raises(RuntimeError):
        H.route_price_table("", R.admitted_cells(R.price_table()) + 1)


def costmap_dict(cost, x0=-5, y0=-3, resolution=0.2, d2=None):
    cost = np.asarray(cost, np.uint8)
    d = dict(x0=x0, y0=y0, nx=cost.shape[1], ny=cost.shape[0], resolution=resolution, inscribed_radius=0.5, inflation_radius=1.0, cost=cost,
             reach=np.zeros_like(cost))
    if d2 is not None:
        d["d2"] = np.asarray(d2, np.uint16)
    return d


def test_the_cell_rule(H):
    c = costmap_dict(pc.empty(12, 9))
    for x, y in ((0, 0), (-0.01, -0.01), (1.39, 1.19), (1.41, 0), (0, -0.61), (float("nan"), 0), (0, float("inf")), (3.0e5, 0), (-1.0, -0.6),
                 (0.6000000001, 0.2), (0.5999999, 0.2), (-0.2, -0.2)):
        assert H.route_cell(c, x, y) == R.cell(x, y, -5, -3, 12, 9, 0.2), (x, y)
    assert H.route_cell(c, 0, 0) == (5, 3) and H.route_cell(c, 1.41, 0) == (-1, -1)


def test_the_summary_and_the_files(H, tmp_path):
    rng = np.random.default_rng(4)
    cost = pc.random_cost(14, 9, 2, 0.1)
    d2 = rng.integers(0, 20, cost.shape).astype(np.uint16)
    d2[rng.random(cost.shape) < 0.5] = 65535
    cells = np.array([[1, 1], [2, 2], [3, 2], [4, 3], [4, 4], [3, 5], [2, 5], [2, 4]], np.int32)
    for with_d2 in (True, False):
        c = costmap_dict(cost, d2=d2 if with_d2 else None)
        got = H.route_summarise(dict(cells=cells), c)
        want = R.summarise(cells, cost, d2 if with_d2 else None, -5, -3, 0.2)
        assert np.array_equal(got["cells"], cells) and np.array_equal(got["xy"], want["xy"])
        assert got["length_m"] == want["length_m"] and got["max_cost"] == want["max_cost"] and got["min_clearance_m"] == want["min_clearance_m"]
        assert with_d2 or got["min_clearance_m"] == -1.0
        prefix = str(tmp_path / ("r%d" % with_d2))
        H.write_route(got, c, prefix)
        assert open(prefix + "_route.txt").read() == R.route_txt(want["xy"])
        assert open(prefix + "_route.pgm", "rb").read() == R.route_pgm_bytes(cost, cells)
    far = costmap_dict(cost, d2=np.full(cost.shape, 65535, np.uint16))
    assert H.route_summarise(dict(cells=cells), far)["min_clearance_m"] == -1.0
    empty = H.route_summarise(dict(cells=np.zeros((0, 2), np.int32)), c)
    assert (empty["length_m"], empty["max_cost"], empty["min_clearance_m"], len(empty["xy"])) == (0.0, 0, -1.0, 0)
    H.write_route(empty, c, str(tmp_path / "none"))
    assert open(str(tmp_path / "none_route.txt")).read() == "" and open(str(tmp_path / "none_route.pgm"), "rb").read() == R.route_pgm_bytes(cost, [])
    for bad in ([[1, 1], [3, 1]], [[1, 1], [1, 1]], [[14, 0]], [[0, -1]]):
        with pytest.raises(RuntimeError):
            H.route_summarise(dict(cells=np.array(bad, np.int32)), c)
    with pytest.raises(RuntimeError):
        H.write_route(got, c, str(tmp_path / "no_such_dir" / "r"))


def test_plan_route_decides_these_without_a_device(H):
    """the four statuses that are settled before a device is asked for, and the refusals of plan_route itself"""
    cost = pc.empty(12, 9)
    cost[3, 5] = 254
    cost[4, 6] = 253
    c = costmap_dict(cost)
    at = lambda col, row: ((-5 + col + 0.5) * 0.2, (-3 + row + 0.5) * 0.2)
    for start, goal, status in ((at(40, 1), at(1, 1), "start_outside"), (at(5, 3), at(1, 1), "start_blocked"), (at(1, 1), (9.0e9, 0.0), "goal_outside"),
                                (at(1, 1), at(6, 4), "goal_blocked"), (at(5, 3), at(40, 1), "start_blocked"), (at(-1, 0), at(6, 4), "start_outside")):
        r = H.plan_route(c, R.route_yaml(start, goal))
        want = R.plan(c, start, goal)
        assert r["status"] == want["status"] == status
        assert r["field"] is None and len(r["cells"]) == 0 and r["cost_to_go"] == R.UNREACHED and r["length_m"] == 0.0 and r["min_clearance_m"] == -1.0
        assert r["start_cell"] == want["start_cell"] and r["goal_cell"] == want["goal_cell"]
    for text in ("", R.route_yaml(at(1, 1), None), R.route_yaml(None, at(1, 1))):
        with pytest.raises(RuntimeError) as e:
            H.plan_route(c, text)
        assert "route:" in str(e.value)
    with pytest.raises(RuntimeError) as e:                                    # the wrap-around bound, before any device
        H.plan_route(costmap_dict(pc.empty(4096, 4096)), R.route_yaml(at(1, 1), at(2, 2), neutral_price=19, cost_factor=0))
    assert "route:" in str(e.value) and str(R.admitted_cells([19])) in str(e.value)
