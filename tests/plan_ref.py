"""A restatement of include/molahip_plan.h and of the host rules of mola_lidar_odometry_hip/RoutePlan.h, written from the two headers
alone: the field by Dijkstra's algorithm with a heap over Python lists, the trace as a plain loop.  Nothing here is shaped like the
device code (no tiles, no sweeps, no relaxation to a fixed point)."""
import heapq
import math

import numpy as np

UNREACHED = 0xFFFFFFFF
TRUNCATED = 0xFFFFFFFF
# the tie order of the trace rule: E, N, W, S, NE, NW, SW, SE as (d column, d row, L)
STEPS = ((1, 0, 5), (0, 1, 5), (-1, 0, 5), (0, -1, 5), (1, 1, 7), (-1, 1, 7), (-1, -1, 7), (1, -1, 7))
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN, PGM_ROUTE = 0, 254, 205, 100


# ---- the device rule ----------------------------------------------------------------------------------------------------------------
def wrap_bound_holds(n_cells, price):
    return (int(n_cells) - 1) * 14 * int(max(int(p) for p in price)) < 0xFFFFFFFF


def _planes(cost, price, passable_below):
    cost = np.asarray(cost, np.uint8)
    price = [int(p) for p in price]
    assert len(price) == passable_below and 1 <= passable_below <= 254 and min(price) >= 1
    ny, nx = cost.shape
    assert wrap_bound_holds(nx * ny, price)
    rows = cost.tolist()
    ok = [[v < passable_below for v in row] for row in rows]
    p = [[price[v] if v < passable_below else 0 for v in row] for row in rows]
    return nx, ny, ok, p


def _allowed(ok, nx, ny, x, y, dx, dy):
    """whether the step (x, y) -> (x + dx, y + dy) exists; (x, y) is passable"""
    u, v = x + dx, y + dy
    if not (0 <= u < nx and 0 <= v < ny) or not ok[v][u]:
        return False
    return dx == 0 or dy == 0 or (ok[y][u] and ok[v][x])


def field(cost, goals_xy, price, passable_below=253):
    """(field uint32 [ny, nx], info dict)"""
    nx, ny, ok, p = _planes(cost, price, passable_below)
    goals = np.asarray(goals_xy, np.int64).reshape(-1, 2).tolist()
    outside = blocked = 0
    dist = [[None] * nx for _ in range(ny)]
    heap = []
    for x, y in goals:
        if not (0 <= x < nx and 0 <= y < ny):
            outside += 1
        elif not ok[y][x]:
            blocked += 1
        elif dist[y][x] is None:
            dist[y][x] = 0
            heap.append((0, x, y))
    done = [[False] * nx for _ in range(ny)]
    while heap:
        d, x, y = heapq.heappop(heap)
        if done[y][x]:
            continue
        done[y][x] = True
        for dx, dy, L in STEPS:
            if _allowed(ok, nx, ny, x, y, dx, dy):
                u, v = x + dx, y + dy
                nd = d + L * (p[y][x] + p[v][u])
                if dist[v][u] is None or nd < dist[v][u]:
                    dist[v][u] = nd
                    heapq.heappush(heap, (nd, u, v))
    out = np.array([[UNREACHED if v is None else v for v in row] for row in dist], np.uint64).astype(np.uint32).reshape(ny, nx)
    finite = out != UNREACHED
    return out, dict(n_reached=int(finite.sum()), max_field=int(out[finite].max()) if finite.any() else 0, n_goals_blocked=blocked,
                     n_goals_outside=outside)


def trace(cost, fld, starts_xy, price, passable_below=253, cap=1 << 30):
    """(a list of int32 [len, 2] routes, the first `cap` cells of a truncated one; the list of lengths, TRUNCATED for those)"""
    nx, ny, ok, p = _planes(cost, price, passable_below)
    f = np.asarray(fld, np.uint32).tolist()
    routes, lens = [], []
    for x, y in np.asarray(starts_xy, np.int64).reshape(-1, 2).tolist():
        if not (0 <= x < nx and 0 <= y < ny) or f[y][x] == UNREACHED:
            routes.append(np.zeros((0, 2), np.int32))
            lens.append(0)
            continue
        cells = [(x, y)]
        while f[y][x] != 0:
            best = None
            for dx, dy, L in STEPS:
                if _allowed(ok, nx, ny, x, y, dx, dy) and f[y + dy][x + dx] != UNREACHED:
                    v = f[y + dy][x + dx] + L * (p[y][x] + p[y + dy][x + dx])
                    if best is None or v < best[0]:          # (strictly: ties go to the first in the order)
                        best = (v, x + dx, y + dy)
            assert best is not None and best[0] == f[y][x], (x, y, best, f[y][x])
            x, y = best[1], best[2]
            cells.append((x, y))
        if len(cells) > cap:
            routes.append(np.array(cells[:cap], np.int32).reshape(-1, 2))
            lens.append(TRUNCATED)
        else:
            routes.append(np.array(cells, np.int32).reshape(-1, 2))
            lens.append(len(cells))
    return routes, lens


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(neutral_price=4, cost_factor=0.08, max_route_cells=1048576)


def price_table(neutral_price=4, cost_factor=0.08, **_):
    t = [int(neutral_price) + int(math.floor(float(cost_factor) * float(c))) for c in range(253)]
    assert max(t) <= 65535
    return np.array(t, np.uint16)


def admitted_cells(price):
    """the largest window, in cells, that the wrap-around bound admits for these prices"""
    return 0xFFFFFFFE // (14 * int(max(int(p) for p in price))) + 1


def cell_of(t, resolution):
    """the floor rule in fp32, un-fused; None when the value has no cell"""
    s = np.float32(t) * (np.float32(1.0) / np.float32(resolution))
    if not np.isfinite(s) or not abs(s) < np.float32(1.0e6):
        return None
    return int(np.floor(s))


def cell(x, y, x0, y0, nx, ny, resolution):
    ix, iy = cell_of(x, resolution), cell_of(y, resolution)
    if ix is None or iy is None or not (0 <= ix - x0 < nx and 0 <= iy - y0 < ny):
        return (-1, -1)
    return (ix - x0, iy - y0)


def summarise(cells, cost, d2, x0, y0, resolution):
    """the route's metres and its summary from its cells (int [n, 2]); d2 may be None"""
    cells = np.asarray(cells, np.int64).reshape(-1, 2).tolist()
    res = float(resolution)
    xy = [((x0 + c + 0.5) * res, (y0 + r + 0.5) * res) for c, r in cells]
    length = 0.0
    for (a, b), (c, r) in zip(cells[:-1], cells[1:]):
        length += res * math.sqrt(2.0) if (a != c and b != r) else res
    near = [int(d2[r][c]) for c, r in cells if int(d2[r][c]) != 65535] if d2 is not None and np.size(d2) else []
    return dict(xy=np.array(xy, np.float64).reshape(-1, 2), length_m=length, max_cost=max([int(cost[r][c]) for c, r in cells], default=0),
                min_clearance_m=math.sqrt(float(min(near))) * res if near else -1.0)


def plan(costmap, start_xy, goal_xy, **options):
    """The whole path on a costmap dict (x0, y0, nx, ny, resolution, cost and optionally d2), in the order of plan_route."""
    opt = dict(DEFAULTS, **options)
    cost = np.asarray(costmap["cost"], np.uint8)
    x0, y0, nx, ny, res = costmap["x0"], costmap["y0"], costmap["nx"], costmap["ny"], costmap["resolution"]
    d2 = costmap.get("d2")
    price = price_table(**opt)
    assert wrap_bound_holds(nx * ny, price)
    s, g = cell(start_xy[0], start_xy[1], x0, y0, nx, ny, res), cell(goal_xy[0], goal_xy[1], x0, y0, nx, ny, res)
    out = dict(start_cell=s, goal_cell=g, cells=np.zeros((0, 2), np.int32), xy=np.zeros((0, 2)), length_m=0.0, cost_to_go=UNREACHED, max_cost=0,
               min_clearance_m=-1.0, field=None, cells_with_field=0)
    if s[0] < 0:
        return dict(out, status="start_outside")
    if cost[s[1], s[0]] >= 253:
        return dict(out, status="start_blocked")
    if g[0] < 0:
        return dict(out, status="goal_outside")
    if cost[g[1], g[0]] >= 253:
        return dict(out, status="goal_blocked")
    f, info = field(cost, [g], price, 253)
    out.update(field=f, cells_with_field=info["n_reached"], cost_to_go=int(f[s[1], s[0]]))
    if f[s[1], s[0]] == UNREACHED:
        return dict(out, status="unreachable")
    cap = min(int(opt["max_route_cells"]), nx * ny)
    routes, lens = trace(cost, f, [s], price, 253, cap)
    out.update(status="truncated" if lens[0] == TRUNCATED else "found", cells=routes[0])
    out.update(summarise(routes[0], cost, d2, x0, y0, res))
    return out


# ---- the files and the yaml ---------------------------------------------------------------------------------------------------------
def route_txt(xy):
    return "".join("%.9g %.9g\n" % (x, y) for x, y in np.asarray(xy, np.float64).reshape(-1, 2).tolist())


def route_pgm_bytes(cost, cells):
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    px = np.where(cost == 255, PGM_UNKNOWN, np.where(cost >= 253, PGM_OCCUPIED, PGM_FREE)).astype(np.uint8)
    for c, r in np.asarray(cells, np.int64).reshape(-1, 2).tolist():
        px[r, c] = PGM_ROUTE
    return b"P5\n%d %d\n255\n" % (nx, ny) + px[::-1].tobytes()


def route_yaml(start_xy=None, goal_xy=None, **keys):
    """the text of a route: block"""
    lines = ["route:"]
    if start_xy is not None:
        lines += ["  start_x: %r" % float(start_xy[0]), "  start_y: %r" % float(start_xy[1])]
    if goal_xy is not None:
        lines += ["  goal_x: %r" % float(goal_xy[0]), "  goal_y: %r" % float(goal_xy[1])]
    lines += ["  %s: %s" % (k, v) for k, v in keys.items()]
    return "\n".join(lines) + "\n" if len(lines) > 1 else ""
