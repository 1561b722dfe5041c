"""Cases for the tests of include/molahip_plan.h and the route planner (tests/test_plan_cpu.py, tests/test_gpu_plan.py).  The planes
are tests/nav_cases.py's, read as cost planes (255 unknown, 254 lethal, 0..253 a cost); what is added here: the price tables, goal
lists, the two-corridor plane where the price decides the route, and the pipeline texts with a route: block."""
import numpy as np

import nav_cases as nc
from nav_cases import LETHAL, UNKNOWN, WINDOWS, diagonal_touch, empty, serpentine, wall  # noqa: F401

BELOW = 253


def stepped(below=BELOW):
    """price 1 + c // 16"""
    return (1 + np.arange(below) // 16).astype(np.uint16)


def flat(below=BELOW, value=1):
    return np.full(below, value, np.uint16)


def by_cost(below=BELOW):
    """price 1 + c"""
    return (1 + np.arange(below)).astype(np.uint16)


def random_cost(nx, ny, seed, lethal):
    """a plane with the given share of lethal cells, a little unknown, costs 0 .. 253 under the rest"""
    return nc.random_base(nx, ny, seed, lethal=lethal, unknown=0.01)


def passable_cells(cost, below=BELOW):
    """int32 [n, 2] of (column, row)"""
    return np.argwhere(np.asarray(cost) < below)[:, ::-1].astype(np.int32)


def blocked_cells(cost, below=BELOW):
    return np.argwhere(np.asarray(cost) >= below)[:, ::-1].astype(np.int32)


def outside_cells(nx, ny):
    return np.array([[-1, 0], [0, -1], [nx, 0], [0, ny], [1 << 30, 3], [-(1 << 31), -(1 << 31)]], np.int32)


def goal_lists(cost, seed):
    """one goal; 50 shuffled goals; goals with blocked and outside ones among them; no goal"""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    rng = np.random.default_rng(seed)
    free, blocked, out = passable_cells(cost), blocked_cells(cost), outside_cells(nx, ny)
    lists = [np.zeros((0, 2), np.int32), out]
    if len(free):
        lists.append(free[rng.integers(0, len(free), 1)])
        lists.append(free[rng.integers(0, len(free), 50)])
        mixed = [free[rng.integers(0, len(free), 5)], out[rng.integers(0, len(out), 4)]]
        if len(blocked):
            mixed.append(blocked[rng.integers(0, len(blocked), 7)])
        mixed = np.concatenate(mixed)
        rng.shuffle(mixed)
        lists.append(mixed)
    if len(blocked):
        lists.append(blocked[:3])
    return lists


def beside_diagonal():
    """a free 5 x 5 plane with one lethal cell at (2, 1): from (1, 1) the diagonal step to (2, 2) passes between (2, 1) and (1, 2), so
    it does not exist, and the way there is two orthogonal steps"""
    b = empty(5, 5)
    b[1, 2] = LETHAL
    return b


def two_corridors(n=9):
    """start (0, 0) and goal (n - 1, 0) in row 0, joined by a straight corridor of cost 250 along row 0 and by a detour of cost 0 up
    column 0, along row 4 and down column n - 1; everything else is lethal"""
    b = empty(n, 5, LETHAL)
    b[0, :] = 250
    b[0, 0] = b[0, n - 1] = 0
    b[:, 0] = 0
    b[:, n - 1] = 0
    b[4, :] = 0
    return b


def scenario_pipeline(inscribed, inflation, unknown_is_obstacle, route_keys=""):
    """the costmap of nav_cases.scenario_pipeline (reached from the first key-frame) with a route: block"""
    return nc.scenario_pipeline(inscribed, inflation, unknown_is_obstacle, "first") + ("route:\n" + route_keys if route_keys else "")
