"""include/molahip_replan.h on the device.  After every update the field is compared bit for bit with tests/plan_ref.py's Dijkstra on
the CURRENT plane, the counters with its info, n_withdrawn with the peeling of tests/replan_ref.py, and routes with plan_ref.trace.
The host path (RoutePlanner, the events text, the command line) is held to plan_ref.plan on the re-inflated costmap of the outdoor
scenario of tests/elev_cases.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi
from mola_lidar_odometry_amd import capi_nav as cn
from mola_lidar_odometry_amd import capi_plan as cp
from mola_lidar_odometry_amd import capi_replan as cr

import nav_cases as nc
import plan_cases as pc
import plan_ref as R
import replan_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


class Case:
    """a plan handle with a valid field, and what the restatements say about it"""

    def __init__(self, ctx, cost, goals, price, below=253):
        self.cost = np.asarray(cost, np.uint8).copy()
        self.ny, self.nx = self.cost.shape
        self.goals, self.price, self.below = np.asarray(goals, np.int32).reshape(-1, 2), price, below
        self.plan = cp.PlanMap(ctx, self.nx, self.ny).set_cost(self.cost).field(self.goals, price, below)
        self.field, _ = R.field(self.cost, self.goals, price, below)
        assert np.array_equal(self.plan.download(), self.field)
        self.n_updates = 0

    def update(self, x0, y0, new, starts=None, do=None):
        """one update of the rectangle at (x0, y0) with the bytes `new` [h, w], checked against the restatements; returns mh_replan_info"""
        new = np.asarray(new, np.uint8)
        before = self.field
        self.cost, changed, repriced = RR.patch(self.cost, x0, y0, new, self.price, self.below)
        if do is None:
            cr.update_cost(self.plan, x0, y0, new)
        else:
            do(self.plan, x0, y0, new)
        self.n_updates += 1
        want, info = R.field(self.cost, self.goals, self.price, self.below)
        got = self.plan.download()
        bad = np.argwhere(got != want)
        assert len(bad) == 0, ("field", self.nx, self.ny, (x0, y0) + new.shape, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        i, ri = self.plan.info(), cr.info(self.plan)
        print("%d x %d, %d x %d at (%d, %d): changed %d repriced %d withdrawn %d; sweeps %d + %d, tile runs %d + %d" % (
            self.nx, self.ny, new.shape[1], new.shape[0], x0, y0, ri.n_cells_changed, ri.n_cells_repriced, ri.n_withdrawn, ri.n_withdraw_sweeps,
            ri.n_relax_sweeps, ri.n_tile_runs_withdraw, ri.n_tile_runs_relax))
        assert (int(i.n_reached), int(i.max_field), int(i.n_goals_blocked), int(i.n_goals_outside)) == \
            (info["n_reached"], info["max_field"], info["n_goals_blocked"], info["n_goals_outside"])
        assert (i.has_cost, i.has_field, i.passable_below) == (1, 1, self.below)
        assert (int(ri.n_cells_changed), int(ri.n_cells_repriced)) == (changed, repriced)
        full = os.environ.get("MH_REPLAN_FULL") is not None
        if not full:
            assert int(ri.n_withdrawn) == RR.n_withdrawn(before, self.cost, self.price, self.below)
        else:
            assert (int(ri.n_withdrawn), ri.n_withdraw_sweeps, int(ri.n_tile_runs_withdraw)) == (0, 0, 0)
        assert (int(i.n_sweeps), int(i.n_tile_runs)) == (ri.n_relax_sweeps, int(ri.n_tile_runs_relax)) and int(ri.n_updates) == self.n_updates
        if repriced == 0:
            assert (ri.n_withdraw_sweeps, ri.n_relax_sweeps, int(ri.n_tile_runs_withdraw), int(ri.n_tile_runs_relax), int(ri.n_withdrawn)) == (0,) * 5
        self.field = want
        if starts is not None:
            routes, lens = R.trace(self.cost, want, starts, self.price, self.below)
            got_routes, got_lens = self.plan.trace(starts, max(max(lens), 1))
            assert got_lens.tolist() == lens
            for a, b in zip(got_routes, routes):
                assert np.array_equal(a, b)
        return ri


def random_rect(rng, nx, ny):
    w, h = int(rng.integers(1, min(nx, 40) + 1)), int(rng.integers(1, min(ny, 40) + 1))
    return int(rng.integers(0, nx - w + 1)), int(rng.integers(0, ny - h + 1)), w, h


# ---- four updates in a row on every window ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", nc.WINDOWS)
def test_every_window(ctx, window):
    """a random plane and a list of goal_lists; then random bytes in a random rectangle, an all-lethal rectangle, a lowering-only one and
    identical bytes, on the one handle"""
    nx, ny = window
    rng = np.random.default_rng(100 * nx + ny)
    cost = pc.random_cost(nx, ny, 10 * nx + ny, 0.1)
    lists = pc.goal_lists(cost, nx + ny)
    for goals in (lists if nx * ny < 1000 else [lists[4 % len(lists)]]):
        price = pc.stepped()
        c = Case(ctx, cost, goals, price)
        starts = rng.integers(0, [nx, ny], (50, 2)).astype(np.int32)
        x0, y0, w, h = random_rect(rng, nx, ny)
        c.update(x0, y0, rng.integers(0, 256, (h, w)).astype(np.uint8), starts)
        x0, y0, w, h = random_rect(rng, nx, ny)
        c.update(x0, y0, np.full((h, w), nc.LETHAL, np.uint8), starts)
        x0, y0, w, h = random_rect(rng, nx, ny)
        old = c.cost[y0:y0 + h, x0:x0 + w]
        lower = np.where(old >= 253, rng.integers(0, 253, (h, w)), old // 2).astype(np.uint8)       # opens cells, lowers prices
        ri = c.update(x0, y0, lower, starts)
        assert int(ri.n_withdrawn) == 0
        x0, y0, w, h = random_rect(rng, nx, ny)
        ri = c.update(x0, y0, c.cost[y0:y0 + h, x0:x0 + w].copy(), starts)
        assert (int(ri.n_cells_changed), ri.n_withdraw_sweeps, ri.n_relax_sweeps, int(ri.n_tile_runs_withdraw), int(ri.n_tile_runs_relax)) == (0,) * 5
        i = c.plan.info()
        assert (i.n_sweeps, i.n_tile_runs) == (0, 0)


def test_the_four_cells_round_a_tile_corner(ctx):
    cost = pc.random_cost(130, 34, 3, 0.05)
    cost[14:18, 62:66] = 0
    c = Case(ctx, cost, [[2, 2], [120, 30]], pc.stepped())
    for x, y in ((63, 15), (64, 15), (63, 16), (64, 16)):
        c.update(x, y, [[nc.LETHAL]], [[60, 14], [67, 18], [63, 15], [64, 16]])
    c.update(63, 15, [[0, 0], [0, 0]], [[60, 14], [67, 18], [63, 15], [64, 16]])
    c.update(63, 15, [[200, nc.LETHAL], [nc.LETHAL, 200]], [[60, 14], [67, 18], [63, 15], [64, 16]])


def test_closing_and_opening_the_gap_of_a_wall(ctx):
    gap = 20
    b = nc.wall(200, 40, 100, gap)
    c = Case(ctx, b, [[3, 3]], pc.flat())
    first = c.field.copy()
    far = int((first[:, 101:] != R.UNREACHED).sum())
    assert far == 99 * 40
    ri = c.update(100, gap, [[nc.LETHAL]], [[150, 5], [50, 5]])
    assert (c.field[:, 100:] == R.UNREACHED).all() and int(ri.n_withdrawn) == far + 1          # the far side and the gap cell itself
    ri = c.update(100, gap, [[0]], [[150, 5], [50, 5]])
    assert np.array_equal(c.field, first) and int(ri.n_withdrawn) == 0


def test_a_diagonal_step_between_two_cells_that_did_not_change(ctx):
    b = pc.beside_diagonal()
    c = Case(ctx, b, [[2, 2]], pc.flat())
    assert c.field[1, 1] == 20
    c.update(2, 1, [[0]], [[1, 1]])
    assert c.field[1, 1] == 14                                                 # the diagonal step exists now
    ri = c.update(2, 1, [[nc.LETHAL]], [[1, 1]])
    assert c.field[1, 1] == 20 and int(ri.n_withdrawn) >= 2                    # (1, 1) rested on the diagonal step, (2, 1) is closed


def test_a_serpentine_blocked_next_to_the_goal(ctx):
    b = pc.serpentine(65)
    c = Case(ctx, b, [[0, 0]], pc.flat())
    n = int((c.field != R.UNREACHED).sum())
    ri = c.update(1, 0, [[nc.LETHAL]], [[64, 64], [0, 0]])
    assert int(ri.n_withdrawn) == n - 1 and ri.n_withdraw_sweeps >= 2 and int(c.plan.info().n_reached) == 1
    ri = c.update(1, 0, [[0]], [[64, 64], [0, 0]])
    assert ri.n_relax_sweeps >= 2 and int(c.plan.info().n_reached) == n


def test_the_price_switches_the_route_and_switches_it_back(ctx):
    b = pc.two_corridors(9)
    b[0, 1:8] = 0
    c = Case(ctx, b, [[8, 0]], pc.by_cost())
    (route,), _ = c.plan.trace([[0, 0]], 64)
    assert route[:, 1].max() == 0
    ri = c.update(1, 0, np.full((1, 7), 250, np.uint8), [[0, 0]])              # the corridor's cost rises until the detour wins
    (route,), _ = c.plan.trace([[0, 0]], 64)
    assert route[:, 1].max() == 4 and int(ri.n_withdrawn) > 0
    assert np.array_equal(c.cost < 253, b < 253)                               # no cell changed its passability
    ri = c.update(1, 0, np.zeros((1, 7), np.uint8), [[0, 0]])
    (route,), _ = c.plan.trace([[0, 0]], 64)
    assert route[:, 1].max() == 0 and int(ri.n_withdrawn) == 0


def test_goals_that_close_and_open(ctx):
    cost = pc.random_cost(90, 50, 4, 0.05)
    cost[10, 10] = 0
    cost[40, 80] = nc.LETHAL
    c = Case(ctx, cost, [[10, 10]], pc.stepped())
    first = c.field.copy()
    c.update(10, 10, [[nc.LETHAL]], [[20, 20]])                                # the only goal blocked
    i = c.plan.info()
    assert (c.field == R.UNREACHED).all() and (int(i.n_reached), int(i.n_goals_blocked)) == (0, 1)
    c.update(10, 10, [[0]], [[20, 20]])
    assert np.array_equal(c.field, first)
    c = Case(ctx, cost, [[10, 10], [80, 40], [80, 40], [-1, 3]], pc.stepped())  # a blocked goal, named twice, and one outside
    assert int(c.plan.info().n_goals_blocked) == 2
    c.update(79, 39, np.zeros((3, 3), np.uint8), [[85, 45], [20, 20]])
    i = c.plan.info()
    assert c.field[40, 80] == 0 and (int(i.n_goals_blocked), int(i.n_goals_outside)) == (0, 1)


# ---- other call shapes --------------------------------------------------------------------------------------------------------------
def test_an_update_before_any_field_and_a_full_window_rectangle(ctx):
    cost = pc.random_cost(70, 40, 9, 0.1)
    plan = cp.PlanMap(ctx, 70, 40).set_cost(cost)
    new = pc.random_cost(30, 20, 10, 0.3)
    cr.update_cost(plan, 5, 7, new)
    ri, i = cr.info(plan), plan.info()
    patched, changed, _ = RR.patch(cost, 5, 7, new, pc.stepped())
    assert (int(ri.n_cells_changed), int(ri.n_cells_repriced), int(ri.n_withdrawn), int(ri.n_updates)) == (changed, 0, 0, 1)
    assert (i.has_cost, i.has_field) == (1, 0)
    goals = [[1, 1], [60, 30]]
    assert np.array_equal(plan.field(goals, pc.stepped()).download(), R.field(patched, goals, pc.stepped())[0])
    assert int(cr.info(plan).n_updates) == 0
    c = Case(ctx, cost, goals, pc.stepped())
    c.update(0, 0, pc.random_cost(70, 40, 11, 0.2), [[3, 3], [50, 20]])        # the whole window: set_cost + field


def test_pinned_and_device_bytes(ctx):
    import torch
    cost = pc.random_cost(300, 260, 8, 0.05)
    new = pc.random_cost(50, 30, 12, 0.4)
    t = torch.from_numpy(new.copy())
    for mem, arr in ((capi.MEM_DEVICE, t.cuda()), (capi.MEM_HOST_PINNED, t.pin_memory())):
        torch.cuda.synchronize()
        c = Case(ctx, cost, [[5, 5], [290, 250]], pc.stepped())
        c.update(100, 90, new, do=lambda plan, x0, y0, b: cr.update_cost(plan, x0, y0, arr.data_ptr(), mem, w=50, h=30))


def test_from_an_mh_nav_after_a_changed_base(ctx):
    nx, ny, R_ = 300, 260, 3
    base = nc.random_base(nx, ny, 31, lethal=0.01, unknown=0.01, costs=False)
    table = nc.ramp_table(R_)
    nav = cn.NavMap(ctx, nx, ny).set_base(base).inflate(R_, table)
    _, cost, _ = nav.download(reach=False)
    below = 200
    goals = pc.passable_cells(cost, below)[[3, 5000]]
    plan = cp.PlanMap(ctx, nx, ny).set_cost_from_nav(nav).field(goals, pc.stepped(below), below)
    base2 = base.copy()
    base2[100:108, 140:170] = nc.LETHAL
    base2[50:60, 30:40] = 0
    # two rectangles of the base change (one call each, grown by the inflation radius and clipped); then one near a corner back
    for rects, b in ((((140, 100, 30, 8), (30, 50, 10, 10)), base2), (((140, 100, 30, 8),), base2), (((0, 0, 5, 5), (140, 100, 30, 8)), base)):
        b = b.copy()
        if len(rects) == 1:
            b[100:108, 140:170] = base[100:108, 140:170]
        if rects[0] == (0, 0, 5, 5):
            b[50:60, 30:40] = 0
            b[0:5, 0:5] = nc.LETHAL
        nav.set_base(b).inflate(R_, table)
        _, cost2, _ = nav.download(reach=False)
        covered = np.zeros((ny, nx), bool)
        for x0, y0, w, h in rects:
            gx, gy, gw, gh = RR.grown_rect(x0, y0, w, h, R_, nx, ny)
            covered[gy:gy + gh, gx:gx + gw] = True
            cr.update_cost_from_nav(plan, nav, gx, gy, gw, gh)
        assert not ((cost2 != cost) & ~covered).any()                          # a base change moves the cost only within R_ cells of it
        want, info = R.field(cost2, goals, pc.stepped(below), below)
        assert np.array_equal(plan.download(), want) and int(plan.info().n_reached) == info["n_reached"]
        cost = cost2
    # the conditions on the mh_nav
    L = cr.lib()
    before = (bytes(plan.info()), bytes(cr.info(plan)))
    fresh = cn.NavMap(ctx, nx, ny).set_base(base)
    other = cn.NavMap(ctx, ny, nx).set_base(base.T.copy()).inflate(R_, table)
    assert L.mh_replan_update_cost_from_nav(plan._h, fresh._h, 0, 0, 4, 4) == 1
    assert L.mh_replan_update_cost_from_nav(plan._h, other._h, 0, 0, 4, 4) == 1
    assert L.mh_replan_update_cost_from_nav(plan._h, None, 0, 0, 4, 4) == 1
    ctx2 = capi.Context(0)
    try:
        elsewhere = cn.NavMap(ctx2, nx, ny).set_base(base).inflate(R_, table)
        assert L.mh_replan_update_cost_from_nav(plan._h, elsewhere._h, 0, 0, 4, 4) == 1
        elsewhere.close()
    finally:
        ctx2.close()
    assert (bytes(plan.info()), bytes(cr.info(plan))) == before and np.array_equal(plan.download(), want)


def test_recomputing_the_whole_field_gives_the_same_bits(ctx, monkeypatch):
    monkeypatch.setenv("MH_REPLAN_FULL", "1")                                  # (read per call)
    c = Case(ctx, nc.wall(200, 40, 100, 20), [[3, 3]], pc.flat())
    c.update(100, 20, [[nc.LETHAL]], [[150, 5]])
    c.update(100, 20, [[0]], [[150, 5]])
    c = Case(ctx, pc.serpentine(65), [[0, 0]], pc.flat())
    c.update(1, 0, [[nc.LETHAL]], [[64, 64]])
    cost = pc.random_cost(300, 260, 10 * 300 + 260, 0.1)
    c = Case(ctx, cost, pc.goal_lists(cost, 560)[4], pc.stepped())
    rng = np.random.default_rng(5)
    c.update(120, 100, rng.integers(0, 256, (33, 40)).astype(np.uint8), [[10, 10], [250, 250]])
    c.update(10, 10, c.cost[10:20, 10:30].copy())                              # identical bytes: no sweep here either


def test_every_refusal_leaves_planes_and_both_infos_as_they_were(ctx):
    L = cr.lib()
    cost = pc.random_cost(40, 30, 6, 0.1)
    new = np.zeros((4, 4), np.uint8)
    empty = cp.PlanMap(ctx, 40, 30)
    assert L.mh_replan_update_cost(empty._h, 0, 0, 4, 4, new.ctypes.data, 0) == 1           # no cost plane
    assert b"cost" in L.mh_last_error_string()
    c = Case(ctx, cost, [[5, 5]], pc.stepped())
    c.update(3, 3, new)
    before = (bytes(c.plan.info()), bytes(cr.info(c.plan)))
    p = new.ctypes.data
    for args in ((0, 0, 4, 4, None, 0), (0, 0, 4, 4, p, 7), (0, 0, 4, 4, p, -1), (0, 0, 0, 4, p, 0), (0, 0, 4, 0, p, 0), (37, 0, 4, 4, p, 0),
                 (0, 27, 4, 4, p, 0), (40, 0, 1, 1, p, 0), (0xFFFFFFFF, 0, 2, 1, p, 0), (0, 0xFFFFFFFE, 1, 4, p, 0), (2, 2, 0xFFFFFFFF, 1, p, 0)):
        assert L.mh_replan_update_cost(c.plan._h, *args) == 1, args
    assert L.mh_replan_update_cost(None, 0, 0, 4, 4, p, 0) == 1 and L.mh_replan_get_info(c.plan._h, None) == 1
    nav = cn.NavMap(ctx, 40, 30).set_base(cost).inflate(1, nc.ramp_table(1))
    for args in ((0, 0, 0, 1), (37, 0, 4, 4), (0, 30, 1, 1), (0xFFFFFFFF, 0, 2, 1)):
        assert L.mh_replan_update_cost_from_nav(c.plan._h, nav._h, *args) == 1, args
    assert L.mh_replan_update_cost_from_nav(empty._h, nav._h, 0, 0, 4, 4) == 1
    assert (bytes(c.plan.info()), bytes(cr.info(c.plan))) == before and np.array_equal(c.plan.download(), c.field)
    c.update(36, 26, new, [[1, 1]])                                            # the last rectangle that fits


def test_a_far_change_runs_fewer_tiles_than_the_field_did(ctx):
    c = Case(ctx, nc.empty(260, 300), [[0, 0]], pc.flat())
    built = int(c.plan.info().n_tile_runs)
    ri = c.update(250, 290, [[nc.LETHAL]], [[259, 299]])
    print("tile runs: the field", built, "the update", int(ri.n_tile_runs_withdraw), "+", int(ri.n_tile_runs_relax))
    assert int(ri.n_tile_runs_withdraw) + int(ri.n_tile_runs_relax) < built


# ---- the host path: the scenario with a lorry across the road -----------------------------------------------------------------------
EVENTS = """# the road of the scenario: from the first key-frame to the last
at 3 0
block 30 -10 31 10     # a lorry across the whole road
at 3 0
clear 30 -3 31 3       # it backs off the carriageway
at 3 0
at 70 0.5
block 200 200 201 201  # nowhere in the window
"""


@pytest.fixture(scope="module")
def scenario():
    import elev_cases as ec
    import elev_ref as ER
    frames, kfset = ec.scenario()
    return frames, kfset, ER.build(frames, **ec.SCENARIO_OPTIONS_DICT)


def restated_run(src, frames, events, **opt):
    """the events on the base plane, the costmap restated from it at every `at`, and plan_ref.plan on that"""
    import nav_ref as NR
    base = np.asarray(src["cost"], np.uint8).copy()
    ny, nx = base.shape
    T = frames[11][1]
    goal = (float(T[3]), float(T[7]))
    routes, rects, outside = [], [], 0
    for verb, v, _ in RR.parse_events(events):
        if verb == "at":
            cm = NR.build(base, src["x0"], src["y0"], 0.2, [T for _, T in frames], reach_from="first", **opt)
            routes.append((R.plan(cm, (v[0], v[1]), goal), cm))
        else:
            rect = RR.metre_rect(v[0], v[1], v[2], v[3], src["x0"], src["y0"], nx, ny, 0.2)
            rects.append(rect)
            if rect is None:
                outside += 1
            else:
                base[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = nc.LETHAL if verb == "block" else 0
    return routes, rects, outside, base


def same_route(r, want):
    assert r["status"] == want["status"]
    assert tuple(r["start_cell"]) == tuple(want["start_cell"]) and tuple(r["goal_cell"]) == tuple(want["goal_cell"])
    assert np.array_equal(r["cells"], want["cells"]) and np.array_equal(r["xy"], want["xy"])
    assert r["cost_to_go"] == want["cost_to_go"] and r["max_cost"] == want["max_cost"] and r["field"] is None
    assert abs(r["length_m"] - want["length_m"]) < 1e-12 and abs(r["min_clearance_m"] - want["min_clearance_m"]) < 1e-12


def test_the_scenario_with_a_block_across_the_road_and_a_clear(scenario, tmp_path):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    opt = dict(inscribed_radius=1.0, inflation_radius=2.0, unknown_is_obstacle=False)
    text = pc.scenario_pipeline(1.0, 2.0, False, "  goal_keyframe: 11\n")
    want, rects, outside, base = restated_run(src, frames, EVENTS, **opt)
    assert [w["status"] for w, _ in want] == ["found", "unreachable", "found", "found"] and outside == 1
    run = H.replan_route_from_keyframes(kfset, text, EVENTS)
    assert len(run["routes"]) == 4 and run["rects_outside"] == 1 and len(run["events"]) == 7 == len(run["summaries"])
    for r, (w, cm) in zip(run["routes"], want):
        assert np.array_equal(r["costmap"]["cost"], cm["cost"]) and np.array_equal(r["costmap"]["d2"], cm["d2"])
        same_route(r, w)
    ups = [e for e in run["events"] if e["verb"] != "at"]
    assert [e["rect"] for e in ups] == rects and ups[2]["rect"] is None
    for e, rect in zip(ups[:2], rects[:2]):
        assert e["grown"] == RR.grown_rect(*rect, 10, src["nx"], src["ny"]) and e["cells_repriced"] > 0       # ceil(2.0 / 0.2) cells
    assert ups[0]["withdrawn"] > 0 and [json.loads(s)["verb"] for s in run["summaries"]] == ["at", "block", "at", "clear", "at", "at", "block"]
    print("block:", run["summaries"][1], "\nclear:", run["summaries"][3])
    assert not np.array_equal(want[0][0]["cells"], want[2][0]["cells"])        # the cleared gap is narrower than the road was: another route
    # the planner itself, a rectangle of bytes at a time
    poses = [T.tolist() for _, T in frames]
    T = frames[11][1]
    planner = H.RoutePlanner(dict(x0=src["x0"], y0=src["y0"], nx=src["nx"], ny=src["ny"], resolution=0.2, cost=src["cost"]), poses,
                             pc.scenario_pipeline(1.0, 2.0, False) + R.route_yaml(None, (float(T[3]), float(T[7]))))
    assert planner.max_cells == 10
    same_route(planner.route_from(3.0, 0.0), want[0][0])
    for rect, byte in ((rects[0], nc.LETHAL), (rects[1], 0)):
        u = planner.update(rect[0], rect[1], np.full((rect[3], rect[2]), byte, np.uint8))
        assert u["rect"] == rect and u["cells_repriced"] > 0
    assert np.array_equal(planner.base(), base) and np.array_equal(planner.costmap()["cost"], want[3][1]["cost"])
    same_route(planner.route_from(3.0, 0.0), want[2][0])
    same_route(planner.route_from(70.0, 0.5), want[3][0])
    assert planner.route_from(500.0, 0.0)["status"] == "start_outside"
    with pytest.raises(RuntimeError):
        planner.update(src["nx"] - 1, 0, np.zeros((1, 2), np.uint8))          # leaves the window
    # the command line: one route file pair per `at`, one line per event
    kf, events, pipeline = str(tmp_path / "kf.bin"), tmp_path / "events.txt", tmp_path / "pipeline.yaml"
    H.write_keyframe_file(kf, kfset)
    events.write_text(EVENTS)
    pipeline.write_text(text)
    out = subprocess.run([CLI, "--replan-route", kf, str(events), str(tmp_path / "cli"), "-c", str(pipeline)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.strip().split("\n")]
    assert len(lines) == 8 and lines[-1]["routes"] == 4 and lines[-1]["rects_outside"] == 1
    assert [l["status"] for l in lines[:-1] if l["verb"] == "at"] == ["found", "unreachable", "found", "found"]
    for k, (w, cm) in enumerate(want):
        assert open(str(tmp_path / "cli") + "_route_%d.txt" % k, "rb").read() == R.route_txt(w["xy"]).encode()
        assert open(str(tmp_path / "cli") + "_route_%d.pgm" % k, "rb").read() == R.route_pgm_bytes(cm["cost"], w["cells"])
    events.write_text("at 3 0\nblock 1 2 3\n")
    bad = subprocess.run([CLI, "--replan-route", kf, str(events), str(tmp_path / "bad")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "events: line 2" in bad.stderr
    assert subprocess.run([CLI, "--replan-route", kf, str(events)], capture_output=True, text=True, timeout=60).returncode == 2
