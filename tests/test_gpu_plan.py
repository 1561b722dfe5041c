"""include/molahip_plan.h on the device.  Every field and every route is compared bit for bit with tests/plan_ref.py, the restatement
written from the header (Dijkstra with a heap, a plain loop for the trace); the host path (key-frames to costmap to route to files,
through pybind and the command line) is held to the same restatement on the outdoor scenario of tests/elev_cases.py, and to the
facts tests/test_gpu_nav.py already pins about it: a vehicle of 1 m radius gets from the first key-frame to the last, one of 2 m
does not when unknown cells count as obstacles, and does -- round the box, where the road simply ends -- when they do not."""
import json
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi
from mola_lidar_odometry_amd import capi_nav as cn
from mola_lidar_odometry_amd import capi_plan as cp

import elev_cases as ec
import elev_ref as ER
import nav_cases as nc
import nav_ref as NR
import plan_cases as pc
import plan_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def field_same(ctx, cost, goals, price, below=253, plan=None):
    """the device's field of a cost plane against the restatement's, and the counters; returns the handle, the field and the info"""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    if plan is None:
        plan = cp.PlanMap(ctx, nx, ny).set_cost(cost)
    plan.field(goals, price, below)
    got = plan.download()
    want, info = R.field(cost, goals, price, below)
    assert got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("field", nx, ny, len(np.asarray(goals).reshape(-1, 2)), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    i = plan.info()
    assert (int(i.n_reached), int(i.max_field), int(i.n_goals_blocked), int(i.n_goals_outside)) == \
        (info["n_reached"], info["max_field"], info["n_goals_blocked"], info["n_goals_outside"])
    assert (i.has_cost, i.has_field, i.passable_below) == (1, 1, below)
    if info["n_reached"] == 0:
        assert i.n_sweeps == 0 and i.n_tile_runs == 0
    else:
        assert i.n_sweeps >= 1 and i.n_tile_runs >= 1
    return plan, want, info


# ---- the field ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", nc.WINDOWS)
def test_every_window(ctx, window):
    """random planes with a lethal share of 0.25 and of 0.02, prices 1 + c // 16 and the constant 1; one goal, 50 shuffled goals, goals
    blocked and outside, no goal.  A small window takes every combination; a large one takes every share with every price and, over
    those four, every kind of goal list at least once (the restatement's heap takes a third of a second per field there)."""
    nx, ny = window
    small = nx * ny < 1000
    k = 0
    for lethal in (0.25, 0.02):
        cost = pc.random_cost(nx, ny, 10 * nx + ny + int(100 * lethal), lethal)
        lists = pc.goal_lists(cost, nx + ny)
        plan = cp.PlanMap(ctx, nx, ny).set_cost(cost)
        for price in (pc.stepped(), pc.flat()):
            for goals in (lists if small else [lists[(2 * k) % len(lists)], lists[(2 * k + 1) % len(lists)]]):
                _, want, _ = field_same(ctx, cost, goals, price, plan=plan)
                if len(goals) > 1:                                                 # the order of the goals plays no part
                    assert np.array_equal(plan.field(goals[::-1], price).download(), want)
            k += 1
        assert small or len(lists) <= 8


def test_walls_with_a_gap_on_and_beside_tile_corners(ctx):
    TX, TY = cp.TILE_X, cp.TILE_Y
    assert (TX, TY) == (64, 16)
    for x, gap in ((70, None), (70, 20), (TX - 1, TY - 1), (TX, TY), (TX, TY - 1), (TX - 1, TY), (2 * TX, 2 * TY), (2 * TX - 1, 2 * TY - 1)):
        b = nc.wall(200, 50, x, gap)                                              # a wall with no gap, with one, with one on a tile corner
        _, f, _ = field_same(ctx, b, [[3, 3]], pc.flat())
        finite = f != R.UNREACHED
        assert finite[:, :x].all() and bool(finite[:, x + 1:].all()) == (gap is not None) and bool(finite[:, x + 1:].any()) == (gap is not None)


def test_windows_that_end_on_a_tile_edge_one_short_and_one_beyond(ctx):
    TX, TY = cp.TILE_X, cp.TILE_Y
    for nx, ny in ((2 * TX + 1, 2 * TY + 1), (2 * TX, 2 * TY), (2 * TX - 1, 2 * TY - 1), (TX + 1, TY + 1), (TX, TY), (TX - 1, TY - 1)):
        cost = pc.random_cost(nx, ny, nx, 0.1)
        free = pc.passable_cells(cost)
        field_same(ctx, cost, free[[0, -1]], pc.stepped())
        field_same(ctx, cost, [[nx - 1, ny - 1], [0, ny - 1], [TX - 1, TY - 1], [TX, TY]], pc.flat())


def test_no_corner_is_cut(ctx):
    _, f, _ = field_same(ctx, pc.diagonal_touch(12), [[2, 2]], pc.flat())
    assert (f[1:6, 1:6] != R.UNREACHED).all() and (f[6:, 6:] == R.UNREACHED).all()     # the second square touches at a corner only
    b = pc.beside_diagonal()
    plan, f, _ = field_same(ctx, b, [[2, 2]], pc.flat())
    assert f[1, 1] == 20 and f[3, 3] == 14                                              # 5 + 5 steps of mean price 1, not one of 7
    (route,), lens = plan.trace([[1, 1]], 10)
    assert lens[0] == 3 and route.tolist() == [[1, 1], [1, 2], [2, 2]]                   # round the lethal cell: N then E (E first is lethal)


def test_a_serpentine_needs_more_than_one_sweep(ctx):
    b = pc.serpentine(65)
    plan, f, info = field_same(ctx, b, [[0, 0]], pc.flat())
    i = plan.info()
    print("serpentine 65 x 65: sweeps", i.n_sweeps, "tile runs", i.n_tile_runs, "max field", i.max_field)
    assert i.n_sweeps >= 2 and ((f != R.UNREACHED) == (b == 0)).all()
    assert int(i.max_field) == info["max_field"] == int(f[64, 64]) == 10 * (33 * 64 + 64)    # every free row end to end, two steps per wall


def test_corridors_of_one_cell(ctx):
    for nx, ny in ((70, 1), (1, 70), (5000, 1)):
        b = nc.empty(nx, ny)
        b.reshape(-1)[50] = nc.LETHAL
        b.reshape(-1)[60:] = 100
        _, f, _ = field_same(ctx, b, [[0, 0]], pc.stepped())
        assert (f.reshape(-1)[:50] == 10 * np.arange(50)).all() and (f.reshape(-1)[50:] == R.UNREACHED).all()
        _, f, info = field_same(ctx, b, [[nx - 1, ny - 1], [0, 0]], pc.stepped())
        assert info["n_reached"] == nx * ny - 1 and f.reshape(-1)[51] == 10 * 8 + 5 * (1 + 7) + 70 * (nx * ny - 61)


def test_the_price_decides_the_route(ctx):
    b = pc.two_corridors(9)
    for price, row in ((pc.by_cost(), 4), (pc.flat(), 0)):
        plan, f, _ = field_same(ctx, b, [[8, 0]], price)
        (route,), lens = plan.trace([[0, 0]], 64)
        (want,), _ = R.trace(b, f, [[0, 0]], price)
        assert np.array_equal(route, want) and lens[0] == len(want)
        assert route[:, 1].max() == row and tuple(route[-1]) == (8, 0)              # the detour over row 4 when cost has a price; else row 0


# ---- the trace ----------------------------------------------------------------------------------------------------------------------
def test_routes_from_200_starts(ctx):
    nx, ny = 300, 260
    cost = pc.random_cost(nx, ny, 77, 0.15)
    price = pc.stepped()
    rng = np.random.default_rng(7)
    free = pc.passable_cells(cost)
    goals = free[rng.integers(0, len(free), 3)]
    plan, f, _ = field_same(ctx, cost, goals, price)
    starts = np.concatenate([free[rng.integers(0, len(free), 190)], pc.blocked_cells(cost)[:4], pc.outside_cells(nx, ny)])
    assert len(starts) == 200
    want, want_len = R.trace(cost, f, starts, price)
    cap = max(want_len)
    got, lens = plan.trace(starts, cap)
    assert lens.tolist() == want_len
    goal_set = {tuple(g) for g in goals.tolist()}
    n_routes = 0
    for s, a, b in zip(starts.tolist(), got, want):
        assert np.array_equal(a, b), s                                            # cell for cell
        if len(a) == 0:
            assert not (0 <= s[0] < nx and 0 <= s[1] < ny) or f[s[1], s[0]] == R.UNREACHED
            continue
        n_routes += 1
        assert tuple(a[0]) == tuple(s) and tuple(a[-1]) in goal_set and f[a[-1, 1], a[-1, 0]] == 0
        fa = f[a[:, 1], a[:, 0]].astype(np.int64)
        pa = price[cost[a[:, 1], a[:, 0]]].astype(np.int64)
        L = np.where((np.diff(a[:, 0]) != 0) & (np.diff(a[:, 1]) != 0), 7, 5)
        assert np.array_equal(fa[:-1] - fa[1:], L * (pa[:-1] + pa[1:]))           # the field falls by exactly w along every step
    assert n_routes >= 150 and lens[190:].tolist() == [0] * 10                    # starts on blocked cells and outside give 0
    # cap equal to a route's length passes; one less truncates with the first cap cells written
    long = [k for k in np.argsort(want_len)[::-1][:3] if want_len[k] > 1]
    for k in long:
        n = want_len[k]
        (route,), ln = plan.trace(starts[k:k + 1], n)
        assert ln[0] == n and np.array_equal(route, want[k])
        (route,), ln = plan.trace(starts[k:k + 1], n - 1)
        assert ln[0] == cp.TRUNCATED and np.array_equal(route, want[k][:n - 1])
    sub = starts[[long[0], 195, long[1]]]                                         # ... and each route of a call on its own
    got, lens = plan.trace(sub, want_len[long[1]])
    assert lens.tolist() == [cp.TRUNCATED if want_len[long[0]] > want_len[long[1]] else want_len[long[0]], 0, want_len[long[1]]]
    assert np.array_equal(got[0], want[long[0]][:want_len[long[1]]]) and np.array_equal(got[2], want[long[1]])
    (route,), ln = plan.trace(goals[:1], 1)                                       # a start on a goal: one cell
    assert ln[0] == 1 and route.tolist() == goals[:1].tolist()
    assert plan.trace(np.zeros((0, 2), np.int32), 5)[0] == []


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def test_every_tile_in_every_sweep_gives_the_same_bits(ctx, monkeypatch):
    cases = [(pc.random_cost(300, 260, 5, 0.02), [[0, 0]], pc.stepped()), (pc.serpentine(65), [[0, 0]], pc.flat())]
    runs = []
    for cost, goals, price in cases:
        plan, _, _ = field_same(ctx, cost, goals, price)
        runs.append((int(plan.info().n_tile_runs), int(plan.info().n_sweeps)))
    monkeypatch.setenv("MH_PLAN_ALL_TILES", "1")                                  # (read per call: the measuring switch)
    for (cost, goals, price), (active, sweeps) in zip(cases, runs):
        plan, _, _ = field_same(ctx, cost, goals, price)
        i = plan.info()
        print("%d x %d: tile runs %d with active tiles (%d sweeps), %d with every tile (%d sweeps)" % (cost.shape[1], cost.shape[0], active,
                                                                                                      sweeps, i.n_tile_runs, i.n_sweeps))
        assert int(i.n_tile_runs) >= active


# ---- with include/molahip_nav.h -----------------------------------------------------------------------------------------------------
def test_the_cost_of_an_mh_nav_and_its_reach_plane(ctx):
    base = nc.random_base(300, 260, 31, lethal=0.03, unknown=0.01, costs=False)
    table = nc.ramp_table(2)
    nav = cn.NavMap(ctx, 300, 260).set_base(base).inflate(2, table)
    _, cost, _ = nav.download(reach=False)
    seeds = np.concatenate([pc.passable_cells(cost, 200)[[3, 5000]], pc.blocked_cells(cost, 200)[:2], pc.outside_cells(300, 260)[:1]])
    below = 200
    nav.reach(seeds, below)
    reach = nav.download(d2=False, cost=False)[2]
    plan = cp.PlanMap(ctx, 300, 260).set_cost_from_nav(nav)
    plan, f, info = field_same(ctx, cost, seeds, pc.stepped(below), below, plan=plan)
    assert np.array_equal(f != R.UNREACHED, reach == 1)                           # the finite cells are mh_nav_reach's plane
    i, ni = plan.info(), nav.info()
    assert (int(i.n_reached), int(i.n_goals_blocked), int(i.n_goals_outside)) == (int(ni.n_reached), int(ni.n_seeds_blocked), int(ni.n_seeds_outside))
    # refusals: an mh_nav without a cost, of another size, of another context; the plan keeps its planes
    L = cp.lib()
    fresh = cn.NavMap(ctx, 300, 260).set_base(base)
    other_size = cn.NavMap(ctx, 260, 300).set_base(base.T.copy()).inflate(2, table)
    assert L.mh_plan_set_cost_from_nav(plan._h, fresh._h) == 1
    assert L.mh_plan_set_cost_from_nav(plan._h, other_size._h) == 1
    assert L.mh_plan_set_cost_from_nav(plan._h, None) == 1
    ctx2 = capi.Context(0)
    try:
        elsewhere = cn.NavMap(ctx2, 300, 260).set_base(base).inflate(2, table)
        assert L.mh_plan_set_cost_from_nav(plan._h, elsewhere._h) == 1
        elsewhere.close()
    finally:
        ctx2.close()
    assert plan.info().has_field == 1 and np.array_equal(plan.download(), f)


def test_pinned_and_device_costs_give_the_same_bits(ctx):
    import torch
    cost = pc.random_cost(300, 260, 8, 0.05)
    goals = [[5, 5], [290, 250]]
    want = R.field(cost, goals, pc.stepped())[0]
    t = torch.from_numpy(cost.copy())
    for mem, arr in ((capi.MEM_DEVICE, t.cuda()), (capi.MEM_HOST_PINNED, t.pin_memory())):
        torch.cuda.synchronize()
        plan = cp.PlanMap(ctx, 300, 260).set_cost(arr.data_ptr(), mem).field(goals, pc.stepped())
        assert np.array_equal(plan.download(), want), mem


# ---- handle state -------------------------------------------------------------------------------------------------------------------
def test_two_handles_and_a_new_cost_invalidates(ctx):
    a_cost, b_cost = pc.random_cost(70, 40, 1, 0.1), pc.random_cost(33, 90, 2, 0.1)
    a, fa, _ = field_same(ctx, a_cost, [[1, 1], [60, 30]], pc.stepped())
    b, fb, _ = field_same(ctx, b_cost, [[2, 2]], pc.flat())
    assert np.array_equal(a.download(), fa) and np.array_equal(b.download(), fb)
    (ra,), _ = a.trace(pc.passable_cells(a_cost)[100:101], 200)
    assert np.array_equal(ra, R.trace(a_cost, fa, pc.passable_cells(a_cost)[100:101], pc.stepped())[0][0])
    a.set_cost(a_cost[::-1].copy())
    i = a.info()
    assert (i.has_cost, i.has_field, i.n_reached, i.n_sweeps, i.max_field) == (1, 0, 0, 0, 0)
    with pytest.raises(capi.MolahipError) as e:
        a.download()
    assert e.value.status == 1
    with pytest.raises(capi.MolahipError) as e:
        a.trace([[1, 1]], 5)
    assert e.value.status == 1
    assert np.array_equal(b.download(), fb)                                       # the other handle has not noticed
    field_same(ctx, a_cost[::-1].copy(), [[1, 38]], pc.stepped(), plan=a)


def test_every_refusal_leaves_the_handle_as_it_was(ctx):
    L = cp.lib()
    C = cp.C
    h = C.c_void_p()
    for nx, ny in ((0, 4), (4, 0), (8193, 8192), (1 << 31, 1)):
        assert L.mh_plan_create(ctx._h, nx, ny, C.byref(h)) == 1 and not h.value
    assert L.mh_plan_create(ctx._h, 4, 4, None) == 1
    plan = cp.PlanMap(ctx, 6, 5)
    cost = pc.random_cost(6, 5, 1, 0.1)
    cost[1, 1] = 0
    price = pc.stepped()
    pp = price.ctypes.data_as(cp._U16P)
    one = np.array([[1, 1]], np.int32)
    gp = one.ctypes.data_as(cp._I32P)
    out = np.zeros((4, 2), np.int32)
    op = out.ctypes.data_as(cp._I32P)
    ln = np.zeros(1, np.uint32)
    lp = ln.ctypes.data_as(cp._U32P)
    f = np.zeros((5, 6), np.uint32)
    fp = f.ctypes.data_as(cp._U32P)
    assert L.mh_plan_field(plan._h, gp, 1, 253, pp, 253) == 1                     # before a cost
    assert b"cost" in L.mh_last_error_string()
    assert L.mh_plan_set_cost(plan._h, None, 0) == 1 and L.mh_plan_set_cost(plan._h, cost.ctypes.data, 7) == 1
    assert plan.info().has_cost == 0
    plan.set_cost(cost)
    assert L.mh_plan_trace(plan._h, gp, 1, 4, op, lp) == 1 and L.mh_plan_download(plan._h, fp) == 1     # before a field
    plan.field(one, price)
    want = R.field(cost, one, price)[0]
    before = bytes(plan.info())
    for below in (0, 255, 1000):
        assert L.mh_plan_field(plan._h, gp, 1, below, pp, below) == 1
    assert L.mh_plan_field(plan._h, gp, 1, 253, pp, 252) == 1 and L.mh_plan_field(plan._h, gp, 1, 252, pp, 253) == 1     # n_price != passable_below
    assert L.mh_plan_field(plan._h, gp, 1, 253, None, 253) == 1 and L.mh_plan_field(plan._h, None, 1, 253, pp, 253) == 1
    for k in (0, 100, 252):
        zero = price.copy()
        zero[k] = 0
        assert L.mh_plan_field(plan._h, gp, 1, 253, zero.ctypes.data_as(cp._U16P), 253) == 1                            # a price of 0
        assert b"price of 0" in L.mh_last_error_string()
    assert L.mh_plan_trace(plan._h, gp, 1, 0, op, lp) == 1                        # cap == 0
    assert L.mh_plan_trace(plan._h, None, 1, 4, op, lp) == 1 and L.mh_plan_trace(plan._h, gp, 1, 4, None, lp) == 1
    assert L.mh_plan_trace(plan._h, gp, 1, 4, op, None) == 1 and L.mh_plan_download(plan._h, None) == 1
    assert L.mh_plan_set_cost(plan._h, cost.ctypes.data, -1) == 1
    assert bytes(plan.info()) == before and np.array_equal(plan.download(), want)                                        # as it was
    (route,), lens = plan.trace(one, 4)
    assert lens[0] == 1 and route.tolist() == [[1, 1]]


def test_the_wrap_around_bound_at_4096_x_4096(ctx):
    plan = cp.PlanMap(ctx, 4096, 4096)
    L = cp.lib()
    for top, status in ((19, 1), (18, 0)):
        price = pc.flat(value=1)
        price[7] = top
        pp = price.ctypes.data_as(cp._U16P)
        assert L.mh_plan_field(plan._h, None, 0, 253, pp, 253) == 1               # no cost yet: both are refused, 19 for the bound
        assert (b"wrap" in L.mh_last_error_string()) == (top == 19)
    plan.set_cost(np.zeros((4096, 4096), np.uint8))
    for top, status in ((19, 1), (18, 0)):
        price = pc.flat(value=1)
        price[7] = top
        assert L.mh_plan_field(plan._h, None, 0, 253, price.ctypes.data_as(cp._U16P), 253) == status
        i = plan.info()
        assert i.has_field == (1 if status == 0 else 0)
    assert (i.n_sweeps, i.n_reached, i.n_tile_runs) == (0, 0, 0)                  # an empty goal list: an all-UNREACHED plane
    f = plan.download()
    assert f.shape == (4096, 4096) and (f == R.UNREACHED).all()


# ---- the host path: the scenario ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    frames, kfset = ec.scenario()
    return frames, kfset, ER.build(frames, **ec.SCENARIO_OPTIONS_DICT)


def restated_costmap(src, frames, **opt):
    return NR.build(src["cost"], src["x0"], src["y0"], 0.2, [T for _, T in frames], reach_from="first", **opt)


def equal_routes(r, want):
    assert r["status"] == want["status"]
    assert tuple(r["start_cell"]) == tuple(want["start_cell"]) and tuple(r["goal_cell"]) == tuple(want["goal_cell"])
    assert (r["field"] is None) == (want["field"] is None)
    if want["field"] is not None:
        assert r["field"].dtype == np.uint32 and np.array_equal(r["field"], want["field"])
    assert np.array_equal(r["cells"], want["cells"]) and np.array_equal(r["xy"], want["xy"])
    assert r["cost_to_go"] == want["cost_to_go"] and r["max_cost"] == want["max_cost"] and r["cells_with_field"] == want["cells_with_field"]
    assert abs(r["length_m"] - want["length_m"]) < 1e-12 and abs(r["min_clearance_m"] - want["min_clearance_m"]) < 1e-12


def ends(frames):
    (_, T0), (_, T11) = frames[0], frames[11]
    return (float(T0[3]), float(T0[7])), (float(T11[3]), float(T11[7]))


@pytest.mark.parametrize("radius,inflation,unknown,status", [(1.0, 2.0, False, "found"), (1.0, 2.0, True, "found"), (2.0, 3.0, True, "unreachable"),
                                                              (2.0, 3.0, False, "found")])
def test_the_scenario_from_the_first_key_frame_to_the_last(scenario, radius, inflation, unknown, status):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    assert len(frames) == 12
    start, goal = ends(frames)
    r = H.plan_route_from_keyframes(kfset, pc.scenario_pipeline(radius, inflation, unknown, "  start_keyframe: 0\n  goal_keyframe: 11\n"))
    cm = restated_costmap(src, frames, inscribed_radius=radius, inflation_radius=inflation, unknown_is_obstacle=unknown)
    assert np.array_equal(r["costmap"]["cost"], cm["cost"]) and np.array_equal(r["costmap"]["d2"], cm["d2"])
    want = R.plan(cm, start, goal)
    equal_routes(r, want)
    print("radius", radius, "unknown_is_obstacle", unknown, ":", r["status"], "cells", len(r["cells"]), "length", r["length_m"], "cost_to_go",
          r["cost_to_go"], "clearance", r["min_clearance_m"], "sweeps", r["sweeps"], "tile runs", r["tile_runs"])
    assert r["status"] == status
    if status == "found":
        assert (cm["cost"][r["cells"][:, 1], r["cells"][:, 0]] < 253).all() and r["max_cost"] < 253       # no route cell the radius forbids
        assert r["cost_to_go"] == want["field"][want["start_cell"][1], want["start_cell"][0]] and len(r["cells"]) >= 2
        if radius == 1.0:
            assert r["min_clearance_m"] >= 1.0
    else:
        assert len(r["cells"]) == 0 and r["cost_to_go"] == R.UNREACHED and r["field"] is not None
    # the defaults name the same two key-frames, and so do the metre keys
    again = H.plan_route_from_keyframes(kfset, pc.scenario_pipeline(radius, inflation, unknown))
    equal_routes(again, want)
    again = H.plan_route(r["costmap"], R.route_yaml(start, goal))
    equal_routes(again, want)


def test_the_scenario_through_the_files_and_the_command_line(scenario, tmp_path):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    start, goal = ends(frames)
    keys = dict(neutral_price=2, cost_factor=0.25)
    text = pc.scenario_pipeline(1.0, 2.0, False) + R.route_yaml(start, goal, **keys)
    cm = restated_costmap(src, frames, inscribed_radius=1.0, inflation_radius=2.0, unknown_is_obstacle=False)
    want = R.plan(cm, start, goal, **keys)
    r = H.plan_route_from_keyframes(kfset, text)
    equal_routes(r, want)
    assert want["status"] == "found"
    prefix = str(tmp_path / "road")
    H.write_route(r, r["costmap"], prefix)
    files = {"_route.txt": R.route_txt(want["xy"]).encode(), "_route.pgm": R.route_pgm_bytes(cm["cost"], want["cells"])}
    for s, b in files.items():
        assert open(prefix + s, "rb").read() == b, s
    H.write_costmap(r["costmap"], prefix)
    pipeline = tmp_path / "pipeline.yaml"
    pipeline.write_text(text)
    out = subprocess.run([CLI, "--plan-route", prefix, str(tmp_path / "cli"), "-c", str(pipeline)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().split("\n")[-1])
    assert line["status"] == "found" and line["cells"] == len(want["cells"]) and line["cost_to_go"] == want["cost_to_go"]
    assert line["max_cost"] == want["max_cost"] and line["cells_with_field"] == want["cells_with_field"] and line["sweeps"] >= 1 and line["tile_runs"] >= 1
    assert abs(line["length_m"] - want["length_m"]) < 1e-5 and line["min_clearance_m"] == -1.0      # (a costmap read back from files has no d2)
    for s, b in files.items():
        assert open(str(tmp_path / "cli") + s, "rb").read() == b, s
    # a cap below the route's length: truncated, the first cells kept
    cut = H.plan_route(r["costmap"], R.route_yaml(start, goal, max_route_cells=10, **keys))
    assert cut["status"] == "truncated" and np.array_equal(cut["cells"], want["cells"][:10])
    bad = subprocess.run([CLI, "--plan-route", prefix, str(tmp_path / "bad")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2                                                    # no pipeline: no start and no goal
