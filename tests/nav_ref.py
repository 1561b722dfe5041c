"""A numpy restatement of include/molahip_nav.h and of the host rules of mola_lidar_odometry_hip/NavCostmap.h, written from the
two headers alone: the distance by brute force over the list of obstacle cells, the flood fill by repeated dilation.  Nothing here
is shaped like the device code (no passes, no tiles, no sweeps)."""
import math

import numpy as np

FAR = 65535
UNKNOWN, LETHAL = 255, 254
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205


# ---- the device rule ----------------------------------------------------------------------------------------------------------------
def obstacles(base, unknown_is_obstacle):
    base = np.asarray(base, np.uint8)
    return (base == LETHAL) | ((base == UNKNOWN) if unknown_is_obstacle else False)


def distance2(base, max_cells, unknown_is_obstacle=False, chunk=1 << 22):
    """uint16 [ny, nx]: the minimum over the obstacle cells of dx^2 + dy^2, FAR where it exceeds max_cells^2 or no obstacle exists.
    Brute force: every cell against every obstacle (only obstacles inside the cell's bounding square can matter, so cells are worked
    per obstacle-free chunk and the obstacle list is cut to the chunk's neighbourhood -- a cut of the list, not another rule)."""
    base = np.asarray(base, np.uint8)
    ny, nx = base.shape
    R = int(max_cells)
    oy, ox = np.nonzero(obstacles(base, unknown_is_obstacle))
    out = np.full((ny, nx), FAR, np.int64)
    if len(ox) == 0:
        return out.astype(np.uint16)
    cy, cx = np.mgrid[0:ny, 0:nx]
    cy, cx = cy.ravel(), cx.ravel()
    best = np.full(ny * nx, np.iinfo(np.int64).max, np.int64)
    per = max(1, chunk // max(1, len(ox)))
    if len(ox) * ny * nx <= chunk * 8:
        for s in range(0, ny * nx, per):
            d = (cx[s:s + per, None] - ox[None, :]) ** 2 + (cy[s:s + per, None] - oy[None, :]) ** 2
            best[s:s + per] = d.min(axis=1)
    else:                                       # many cells and many obstacles: obstacle by obstacle over its square of side 2 R + 1
        best2 = best.reshape(ny, nx)
        for x, y in zip(ox.tolist(), oy.tolist()):
            x0, x1, y0, y1 = max(0, x - R), min(nx, x + R + 1), max(0, y - R), min(ny, y + R + 1)
            d = (np.arange(x0, x1)[None, :] - x) ** 2 + (np.arange(y0, y1)[:, None] - y) ** 2
            np.minimum(best2[y0:y1, x0:x1], d, out=best2[y0:y1, x0:x1])
    best = best.reshape(ny, nx)
    return np.where(best <= R * R, best, FAR).astype(np.uint16)


def inflate(base, max_cells, table, unknown_is_obstacle=False):
    """(d2 uint16, cost uint8)"""
    base = np.asarray(base, np.uint8)
    table = np.asarray(table, np.uint8)
    assert len(table) == max_cells * max_cells + 1 and (table <= 253).all()
    d2 = distance2(base, max_cells, unknown_is_obstacle)
    t = np.where(d2 == FAR, 0, table[np.minimum(d2, len(table) - 1)])
    cost = np.where(base >= LETHAL, base, np.maximum(base, t)).astype(np.uint8)
    return d2, cost


def reach(cost, seeds_xy, passable_below):
    """(reach uint8 [ny, nx], info dict)"""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    passable = cost < passable_below
    seeds = np.asarray(seeds_xy, np.int64).reshape(-1, 2)
    inside = (seeds[:, 0] >= 0) & (seeds[:, 0] < nx) & (seeds[:, 1] >= 0) & (seeds[:, 1] < ny)
    on = seeds[inside]
    ok = passable[on[:, 1], on[:, 0]]
    r = np.zeros((ny, nx), bool)
    r[on[ok, 1], on[ok, 0]] = True
    while True:
        grown = r.copy()
        grown[1:, :] |= r[:-1, :]
        grown[:-1, :] |= r[1:, :]
        grown[:, 1:] |= r[:, :-1]
        grown[:, :-1] |= r[:, 1:]
        grown &= passable
        if (grown == r).all():
            break
        r = grown
    return r.astype(np.uint8), dict(n_reached=int(r.sum()), n_seeds_blocked=int((~ok).sum()), n_seeds_outside=int((~inside).sum()))


def components_of(cost, seeds_xy, passable_below):
    """the same set by labelling: a check of the dilation loop on small planes (a breadth-first walk from the seeds)"""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    passable = cost < passable_below
    r = np.zeros((ny, nx), np.uint8)
    todo = [(int(x), int(y)) for x, y in np.asarray(seeds_xy, np.int64).reshape(-1, 2) if 0 <= x < nx and 0 <= y < ny and passable[y, x]]
    for x, y in todo:
        r[y, x] = 1
    while todo:
        x, y = todo.pop()
        for u, v in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= u < nx and 0 <= v < ny and passable[v, u] and not r[v, u]:
                r[v, u] = 1
                todo.append((u, v))
    return r


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(source="traversability", inscribed_radius=0.5, inflation_radius=1.5, cost_scaling=3.0, unknown_is_obstacle=False,
                reach_from="keyframes")


def max_cells(inflation_radius, resolution):
    return int(math.ceil(float(inflation_radius) / float(resolution)))


def table(resolution, inscribed_radius=0.5, inflation_radius=1.5, cost_scaling=3.0, **_):
    R = max_cells(inflation_radius, resolution)
    t = np.zeros(R * R + 1, np.uint8)
    for d2 in range(1, R * R + 1):
        d = math.sqrt(float(d2)) * float(resolution)
        if d <= inscribed_radius:
            t[d2] = 253
        elif d <= inflation_radius:
            t[d2] = int(math.floor(252.0 * math.exp(-cost_scaling * (d - inscribed_radius))))
    return t


def base_of_grid(cells):
    cells = np.asarray(cells, np.int8)
    return np.where(cells == 100, LETHAL, np.where(cells == -1, UNKNOWN, 0)).astype(np.uint8)


def cell_of(t, resolution):
    """the floor rule in fp32, un-fused; None when the translation has no cell"""
    s = np.float32(t) * (np.float32(1.0) / np.float32(resolution))
    if not np.isfinite(s) or not abs(s) < np.float32(1.0e6):
        return None
    return int(np.floor(s))


def seeds(poses, x0, y0, nx, ny, resolution, reach_from="keyframes"):
    """int32 [n, 2] of (column, row) relative to the window; (-1, -1) for a pose without a cell in the window"""
    poses = list(poses)
    poses = [] if reach_from == "none" else poses[:1] if reach_from == "first" else poses
    out = []
    for T in poses:
        ix, iy = cell_of(T[3], resolution), cell_of(T[7], resolution)
        if ix is None or iy is None or not (0 <= ix - x0 < nx and 0 <= iy - y0 < ny):
            out.append((-1, -1))
        else:
            out.append((ix - x0, iy - y0))
    return np.array(out, np.int32).reshape(-1, 2)


def build(base, x0, y0, resolution, poses, **options):
    """The whole path on a base plane, in the order of build_costmap.  Returns a dict with the keys of the host's costmap."""
    opt = dict(DEFAULTS, **options)
    base = np.asarray(base, np.uint8)
    ny, nx = base.shape
    R = max_cells(opt["inflation_radius"], resolution)
    d2, cost = inflate(base, R, table(resolution, **opt), opt["unknown_is_obstacle"])
    r, info = reach(cost, seeds(poses, x0, y0, nx, ny, resolution, opt["reach_from"]), 253)
    out = dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=resolution, max_cells=R, d2=d2, cost=cost, reach=r,
               inscribed_radius=opt["inscribed_radius"], inflation_radius=opt["inflation_radius"],
               seeds_blocked=info["n_seeds_blocked"], seeds_outside=info["n_seeds_outside"])
    out.update(summarise(d2, cost, r, x0, y0, resolution, poses))
    return out


def summarise(d2, cost, r, x0, y0, resolution, poses):
    ny, nx = cost.shape
    below = cost < 253
    out = dict(cells_unknown=int((cost == 255).sum()), cells_lethal=int((cost == 254).sum()), cells_inscribed=int((cost == 253).sum()),
               cells_inflated=int((below & (d2 != FAR)).sum()), cells_free=int((below & (d2 == FAR)).sum()), cells_reached=int((r == 1).sum()),
               cells_unreachable_free=int((below & (r == 0)).sum()))
    kd, kc, kr = [], [], []
    for c, w in seeds(poses, x0, y0, nx, ny, resolution):
        inside = c >= 0
        kd.append(int(d2[w, c]) if inside else FAR)
        kc.append(int(cost[w, c]) if inside else 255)
        kr.append(int(r[w, c]) if inside else 0)
    near = [v for v in kd if v != FAR]
    out.update(keyframe_d2=kd, keyframe_cost=kc, keyframe_reached=kr, keyframes_blocked=sum(1 for v in kc if v >= 253),
               trajectory_min_clearance_m=math.sqrt(float(min(near))) * float(resolution) if near else -1.0)
    return out


# ---- the files ----------------------------------------------------------------------------------------------------------------------
def trinary_pgm_bytes(cost):
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    px = np.where(cost == UNKNOWN, PGM_UNKNOWN, np.where(cost >= 253, PGM_OCCUPIED, PGM_FREE)).astype(np.uint8)
    return b"P5\n%d %d\n255\n" % (nx, ny) + px[::-1].tobytes()


def cost_pgm_bytes(cost):
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    return b"P5\n%d %d\n255\n" % (nx, ny) + cost[::-1].tobytes()


def reach_pgm_bytes(r):
    r = np.asarray(r, np.uint8)
    ny, nx = r.shape
    return b"P5\n%d %d\n255\n" % (nx, ny) + np.where(r[::-1] != 0, 255, 0).astype(np.uint8).tobytes()


def yaml_text(prefix_name, resolution, x0, y0, inscribed_radius, inflation_radius):
    return ("image: %s.pgm\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
            "cost_image: %s_cost.pgm\nreach_image: %s_reach.pgm\ninscribed_radius: %.9g\ninflation_radius: %.9g\n"
            % (prefix_name, resolution, x0 * float(resolution), y0 * float(resolution), prefix_name, prefix_name, inscribed_radius,
               inflation_radius))
